"""The attention kernel alone on a recipe-size layer: 1024-wide TDNN layers around ONE attention-relu-renorm-layer (15 heads, key-dim
40, value-dim 80, 5 left and 2 right inputs, time-stride 3: 2520 input and 1320 output columns), 2 000 pdfs, on the headline batch
geometry.  Times, for a batch of 256 x 3 s and for one 3 s utterance, on samples resident in HBM: the whole un-overlapped decode call
(host clock around the synchronous call) and its acoustic-model stage (rs_result_timings, device events), after a warm-up of every
shape; with --trace the script runs itself once more under `rocprofv3 --kernel-trace --stats` (a run of its own; its files go to the
directory named by --out=DIR, a temporary one by default) and prints the row of the kernel statistics that belongs to
AttentionKernel (one launch per call) with the bytes the layer must move at least -- every input row read once, every output row
written once -- and the fraction of the HBM peak (8 TB/s) the average launch of the batch shape reaches on them.  There is nothing to
compare with: the commit before refuses the model.  Needs the GPU.
  usage: python profiles/micro/attention_times.py [rounds, default 10] [--trace [--out=DIR]]"""
import csv
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from rhasspy_speech_amd import _lib, synth  # noqa: E402
from tests import configs  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
rounds = int(args[0]) if args else 10
if not torch.cuda.is_available():
    raise SystemExit("attention_times.py needs an MI355X")

LAYERS = ((0,), (-1, 0, 1), (-1, 0, 1), (-3, 0, 3), (-3, 0, 3))
LAYER = dict(after=3, heads=15, key_dim=40, value_dim=80, left=5, right=2, stride=3)
HBM_PEAK = 8.0e12
_, IN_DIM, OUT_DIM = synth.attention_layer_dims(LAYER)
BATCH_ROWS = 256 * 298      # frames of 256 clips of 3 s (the rows of their context come on top)
MIN_BYTES = BATCH_ROWS * (IN_DIM + OUT_DIM) * 4

if "--trace" in sys.argv[1:]:
    named = [a[len("--out="):] for a in sys.argv[1:] if a.startswith("--out=")]
    out = Path(named[0]) if named else Path(tempfile.mkdtemp(prefix="rs_attention_trace_"))
    out.mkdir(parents=True, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", str(out), "-o", "attention", "--output-format", "csv", "--",
           sys.executable, str(Path(__file__).resolve()), "3", "--batch-only"]
    rc = subprocess.run(cmd, timeout=900).returncode
    for f in sorted(out.rglob("*kernel_stats.csv")):
        with open(f, newline="") as fh:
            rows = list(csv.DictReader(fh))
        total = sum(float(r.get("TotalDurationNs", 0) or 0) for r in rows)
        for r in rows:
            if "AttentionKernel" in r.get("Name", ""):
                avg = float(r.get("AverageNs", 0)) / 1e9
                print(f"trace (3 timed rounds + warm-up, 256 x 3 s): {r['Name'][:60]}: calls {r.get('Calls')}, total {float(r['TotalDurationNs']) / 1e6:.2f} ms, "
                      f"average {avg * 1e3:.3f} ms, min {float(r.get('MinNs', 0)) / 1e6:.3f} ms, {100 * float(r['TotalDurationNs']) / max(total, 1):.1f} % of all kernel time; "
                      f"at least {MIN_BYTES / 1e9:.3f} GB to move ({BATCH_ROWS} rows x ({IN_DIM} + {OUT_DIM}) floats): {MIN_BYTES / max(avg, 1e-12) / 1e12:.2f} TB/s, "
                      f"{100 * MIN_BYTES / max(avg, 1e-12) / HBM_PEAK:.1f} % of the HBM peak")
    sys.exit(rc)

pcms = configs.grammar_utterances(256, 0)


def resident(p):
    return torch.from_numpy(np.concatenate(p)).to("cuda:0"), np.concatenate([[0], np.cumsum([len(x) for x in p])]).astype(np.int64)


spec = synth.ModelSpec(name="tdnn-attention", hidden_dim=1024, prefinal_dim=256, layer_offsets=LAYERS, dither=0.0, attention_layers=(LAYER,))
with tempfile.TemporaryDirectory(prefix="rs_attention_time_") as td:
    synth.write_model_dir(Path(td) / "model", spec)
    synth.make_grammar_graph(Path(td) / "graph", spec, seed=11)
    model = _lib.Model(Path(td) / "model", Path(td) / "graph", _lib.default_opts(device_id=0))
    model.to_device()
    for line in model.describe().splitlines():
        if line.startswith(("attention:", "nnet:")):
            print(line)
    shapes = (("256 x 3 s", pcms),) if "--batch-only" in sys.argv[1:] else (("256 x 3 s", pcms), ("1 x 3 s", pcms[:1]))
    for label, batch in shapes:
        d_pcm, offsets = resident(batch)
        for _ in range(3):      # warm-up: code objects, arenas, a repetition on the exact kernels if the first call asks for one
            model.decode_batch_device(d_pcm.data_ptr(), offsets)
        wall, am = [], []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = model.decode_batch_device(d_pcm.data_ptr(), offsets)
            wall.append((time.perf_counter() - t0) * 1e3)
            am.append(float(res.timings()[3]))
            res.close()
        print(f"attention-relu-renorm, {label}: {rounds} calls: whole call min {min(wall):.2f} ms, median {sorted(wall)[len(wall) // 2]:.2f} ms; "
              f"acoustic-model stage min {min(am):.2f} ms, median {sorted(am)[len(am) // 2]:.2f} ms")
    del model
