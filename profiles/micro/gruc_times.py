"""The two recurrent kernels of the composed GRU forms alone on a recipe-size block: pgru_times.py's net (1024-wide TDNN layers,
2 000 pdfs) around ONE composed block of cell 1024, recurrent 256, non-recurrent 256, delay 3 -- pgru-layer / norm-pgru-layer
(PgrucKernel), opgru-layer / norm-opgru-layer (GrucKernel) -- and around ONE fast-pgru / fast-opgru block of the same dims as the
yardsticks (PgruKernel, GruKernel: the walks do the same products), on the headline batch geometry.  Times, for a batch of 256 x 3 s and for one 3 s utterance, on samples resident in HBM: the whole un-overlapped
decode call (host clock around the synchronous call) and its acoustic-model stage (rs_result_timings, device events), after a
warm-up of every shape; with --trace the script runs itself once more under `rocprofv3 --kernel-trace --stats` (a run of its own;
its files go to the directory named by --out=DIR, a temporary one by default) and prints the rows of the kernel statistics that
belong to the recurrent stage (one launch per call, 110 steps; --only=VARIANT keeps the variants apart: one trace run per variant).
Needs the GPU.
  usage: python profiles/micro/gruc_times.py [rounds, default 10] [--only=pgru|norm-pgru|opgru|norm-opgru|fast-pgru|fast-opgru] [--trace [--out=DIR]]"""
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
    raise SystemExit("gruc_times.py needs an MI355X")

if "--trace" in sys.argv[1:]:
    named = [a[len("--out="):] for a in sys.argv[1:] if a.startswith("--out=")]
    out = Path(named[0]) if named else Path(tempfile.mkdtemp(prefix="rs_gruc_trace_"))
    out.mkdir(parents=True, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", str(out), "-o", "gruc", "--output-format", "csv", "--",
           sys.executable, str(Path(__file__).resolve()), "3"] + [a for a in sys.argv[1:] if a.startswith("--only=")]
    rc = subprocess.run(cmd, timeout=900).returncode
    for f in sorted(out.rglob("*kernel_stats.csv")):
        with open(f, newline="") as fh:
            rows = list(csv.DictReader(fh))
        total = sum(float(r.get("TotalDurationNs", 0) or 0) for r in rows)
        for r in rows:
            if "gru" in r.get("Name", "").lower():
                print(f"trace (3 timed rounds + warm-up, both shapes): {r['Name'][:60]}: calls {r.get('Calls')}, total {float(r['TotalDurationNs']) / 1e6:.2f} ms, "
                      f"average {float(r.get('AverageNs', 0)) / 1e6:.3f} ms, {100 * float(r['TotalDurationNs']) / max(total, 1):.1f} % of all kernel time")
    # the launches one by one (the two shapes differ in their grid): kernel, workgroups, duration
    for f in sorted(out.rglob("*kernel_trace.csv")):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "gru" in r.get("Kernel_Name", "").lower():
                    grid, wg = float(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), float(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 512)) or 512)
                    print(f"launch: {r['Kernel_Name'][:40]}: {int(grid / max(wg, 1))} workgroups, "
                          f"{(float(r['End_Timestamp']) - float(r['Start_Timestamp'])) / 1e6:.3f} ms")
    sys.exit(rc)

LAYERS = ((0,), (-1, 0, 1), (-1, 0, 1), (-3, 0, 3), (-3, 0, 3))
BLOCK = dict(after=3, cell=1024, rec=256, nonrec=256, delay=3)
pcms = configs.grammar_utterances(256, 0)


def resident(p):
    return torch.from_numpy(np.concatenate(p)).to("cuda:0"), np.concatenate([[0], np.cumsum([len(x) for x in p])]).astype(np.int64)


only = [a[len("--only="):] for a in sys.argv[1:] if a.startswith("--only=")]
COMPOSED = dict(BLOCK, form="composed")
for variant, layers in (("pgru", dict(pgru_layers=(COMPOSED,))), ("norm-pgru", dict(pgru_layers=(dict(COMPOSED, norm=True),))),
                        ("opgru", dict(gru_layers=(COMPOSED,))), ("norm-opgru", dict(gru_layers=(dict(COMPOSED, norm=True),))),
                        ("fast-pgru", dict(pgru_layers=(BLOCK,))), ("fast-opgru", dict(gru_layers=(BLOCK,)))):
    if only and variant not in only:
        continue
    spec = synth.ModelSpec(name="tdnn-gruc", hidden_dim=1024, prefinal_dim=256, layer_offsets=LAYERS, dither=0.0, **layers)
    with tempfile.TemporaryDirectory(prefix="rs_gruc_time_") as td:
        synth.write_model_dir(Path(td) / "model", spec)
        synth.make_grammar_graph(Path(td) / "graph", spec, seed=11)
        model = _lib.Model(Path(td) / "model", Path(td) / "graph", _lib.default_opts(device_id=0))
        model.to_device()
        for line in model.describe().splitlines():
            if line.startswith(("pgru:", "gru:", "nnet:")):
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
