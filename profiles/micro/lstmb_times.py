"""The recurrent kernel of an lstmb-layer block alone on recipe-size blocks: 1024-wide TDNN layers around ONE lstmb-layer block, 2 000
pdfs, at the wsj recipe's dims (cell 384, bottleneck 256, delay 3: run_tdnn_lstm_1b.sh) and at cell 1024 / bottleneck 256, and the
same net around ONE fast-lstm-layer block of the same cell dim as the yardstick (LstmKernel without a projection: one product of
4 cell x cell per step where the lstmb block has bottleneck x cell and 4 cell x bottleneck), in the same session, on the headline
batch geometry.  Times, for a batch of 256 x 3 s and for one 3 s utterance, on samples resident in HBM: the whole un-overlapped
decode call (host clock around the synchronous call) and its acoustic-model stage (rs_result_timings, device events), after a
warm-up of every shape; with --trace the script runs itself once more under `rocprofv3 --kernel-trace --stats` (a run of its own;
its files go to the directory named by --out=DIR, a temporary one by default) and prints the launches of the recurrent stage one by
one (LstmbKernel / LstmKernel: one launch per call, 110 steps; --only=VARIANT keeps the variants apart).
Needs the GPU.
  usage: python profiles/micro/lstmb_times.py [rounds, default 10] [--only=lstmb-384|fast-lstm-384|lstmb-1024|fast-lstm-1024] [--trace [--out=DIR]]"""
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
    raise SystemExit("lstmb_times.py needs an MI355X")

if "--trace" in sys.argv[1:]:
    named = [a[len("--out="):] for a in sys.argv[1:] if a.startswith("--out=")]
    out = Path(named[0]) if named else Path(tempfile.mkdtemp(prefix="rs_lstmb_trace_"))
    out.mkdir(parents=True, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", str(out), "-o", "lstmb", "--output-format", "csv", "--",
           sys.executable, str(Path(__file__).resolve()), "3"] + [a for a in sys.argv[1:] if a.startswith("--only=")]
    rc = subprocess.run(cmd, timeout=900).returncode
    # the launches one by one (the variants follow each other in the order below, 256 x 3 s before 1 x 3 s; the two shapes differ in
    # their grid): kernel, workgroups, duration
    for f in sorted(out.rglob("*kernel_trace.csv")):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "lstm" in r.get("Kernel_Name", "").lower():
                    grid, wg = float(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), float(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 512)) or 512)
                    print(f"launch: {r['Kernel_Name'][:40]}: {int(grid / max(wg, 1))} workgroups, "
                          f"{(float(r['End_Timestamp']) - float(r['Start_Timestamp'])) / 1e6:.3f} ms")
    sys.exit(rc)

LAYERS = ((0,), (-1, 0, 1), (-1, 0, 1), (-3, 0, 3), (-3, 0, 3))
VARIANTS = (("lstmb-384", dict(after=3, cell=384, bottleneck=256, delay=3, scale=0.85)),
            ("fast-lstm-384", dict(after=3, cell=384, rec=0, nonrec=0, delay=3, scale=0.85)),
            ("lstmb-1024", dict(after=3, cell=1024, bottleneck=256, delay=3)),
            ("fast-lstm-1024", dict(after=3, cell=1024, rec=0, nonrec=0, delay=3)))
pcms = configs.grammar_utterances(256, 0)


def resident(p):
    return torch.from_numpy(np.concatenate(p)).to("cuda:0"), np.concatenate([[0], np.cumsum([len(x) for x in p])]).astype(np.int64)


only = [a[len("--only="):] for a in sys.argv[1:] if a.startswith("--only=")]
for variant, block in VARIANTS:
    if only and variant not in only:
        continue
    spec = synth.ModelSpec(name="tdnn-lstmb", hidden_dim=1024, prefinal_dim=256, layer_offsets=LAYERS, dither=0.0, lstm_layers=(block,))
    with tempfile.TemporaryDirectory(prefix="rs_lstmb_time_") as td:
        synth.write_model_dir(Path(td) / "model", spec)
        synth.make_grammar_graph(Path(td) / "graph", spec, seed=11)
        model = _lib.Model(Path(td) / "model", Path(td) / "graph", _lib.default_opts(device_id=0))
        model.to_device()
        for line in model.describe().splitlines():
            if line.startswith(("lstmb:", "lstm:", "nnet:")):
                print(line)
        for label, batch in (("256 x 3 s", pcms), ("1 x 3 s", pcms[:1])):
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
            print(f"{variant}, {label}: {rounds} calls: whole call min {min(wall):.2f} ms, median {sorted(wall)[len(wall) // 2]:.2f} ms; "
                  f"acoustic-model stage min {min(am):.2f} ms, median {sorted(am)[len(am) // 2]:.2f} ms")
        del model
