"""The feature kernel's time per frame at the four transform sizes it is instantiated for -- 256, 512, 1024 and 2048 points -- on the
same rows in one session: tiny models (no extractor) at 8, 16, 32 and 48 kHz, whose 25 ms windows (200, 400, 800 and 1200 samples, all
even: the paired loads) pad to those sizes, batches of N utterances of 298 frames each, N = 4, 64 and 384 (1.2 k, 19 k and 115 k frames:
below, inside and above the range in which the launcher gives the 512-point window its 16-wave form with the plan in LDS).
Kernel times come from a kernel trace (one call in flight, warm, the trace in a run of its own), as profiles/collect.sh takes them:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/micro/mfcc_fft_sizes.py
  python profiles/micro/mfcc_fft_sizes.py --read OUT
The second command prints, per kernel instantiation and grid, the median of the timed dispatches and that time per frame."""
import csv
import re
import sys
import tempfile
from collections import defaultdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

RATES = (8000, 16000, 32000, 48000)
UTTS = (4, 64, 384)
FRAMES, CALLS = 298, 7      # per (rate, batch): one warm call, six timed


def read(out_dir: str) -> None:
    rows = defaultdict(list)
    for f in Path(out_dir).rglob("*kernel_trace.csv"):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if not re.search(r"(Mfcc|Fbank)Kernel", r["Kernel_Name"]):
                    continue
                name = re.search(r"(?:Mfcc|Fbank)Kernel<[^>]*>", r["Kernel_Name"]).group(0)
                rows[(name, int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"]))].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for (name, grid, wg), v in sorted(rows.items(), key=lambda kv: (kv[0][1] // 64 > 3000, kv[0][1] // 64 > 40000, kv[0][0])):
        d = sorted(e - s for s, e in sorted(v)[1:])      # (the first dispatch of a grid: cold)
        med = d[len(d) // 2] / 1e3
        print(f"{name:28s} grid {grid // wg:6d} x {wg:4d}  {len(d)} timed  median {med:8.1f} us  min {d[0] / 1e3:8.1f} us  {1e3 * med / (grid // 64):7.2f} ns/row")


def main() -> None:
    import torch
    from rhasspy_speech_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("mfcc_fft_sizes.py needs an MI355X")
    with tempfile.TemporaryDirectory(prefix="rs_fft_sizes_") as td:
        for rate in RATES:
            band = dict(low_freq=40, high_freq=-200) if rate == 8000 else {}
            spec = synth.tiny_spec(ivector_dim=0, sample_frequency=rate, **band)
            root = Path(td) / str(rate)
            synth.write_model_dir(root / "model", spec)
            synth.make_grammar_graph(root / "graph", spec)
            model = _lib.Model(root / "model", root / "graph", _lib.default_opts(device_id=0))
            model.to_device()
            win, shift = int(rate * 0.025), int(rate * 0.010)
            n = win + (FRAMES - 1) * shift
            for utts in UTTS:
                pcm = np.concatenate([synth.synth_utterance(u % 16, n, rate) for u in range(utts)] + [np.zeros(4096, np.int16)])
                d_pcm = torch.from_numpy(pcm).to("cuda:0")
                offsets = (np.arange(utts + 1) * n).astype(np.int64)
                for _ in range(CALLS):
                    res = model.decode_batch_device(d_pcm.data_ptr(), offsets)
                    assert res.num_frames(utts - 1) == FRAMES
                torch.cuda.synchronize()
                print(f"{rate} Hz: window {win}, {utts} x {FRAMES} frames, feature stage of the last call {float(res.timings()[1]) * 1e3:.0f} us", flush=True)
                res.close()
            model.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--read":
        read(sys.argv[2])
    else:
        main()
