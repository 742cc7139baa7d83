"""Partial results on the streams workload: 64 concurrent 30 s streams (bench.py's `streams` audio and model) handed over in 1 s
rounds, each round followed by rs_streams_advance (--mode advance) or by rs_streams_partial over all streams (--mode partial), then
rs_streams_finish.  Prints one JSON line: ms per step (open .. finish), the back-pointer rows the partials read per call, and
whether the finished results equal those of the advance-only run (--mode both runs the two and compares them).
usage (GPU box): python profiles/micro/stream_partial.py --mode both
       rocprofv3 --kernel-trace --stats -d <dir> -o partial -- python profiles/micro/stream_partial.py --mode partial --steps 2"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rhasspy_speech_amd import _lib  # noqa: E402
from tests import configs  # noqa: E402


def step(model, pcms, round_samples, partial):
    streams = [_lib.Stream(model) for _ in pcms]
    rows, calls = 0, 0
    for k in range(0, max(len(p) for p in pcms), round_samples):
        live = [(s, p[k:k + round_samples]) for s, p in zip(streams, pcms) if k < len(p)]
        _lib.accept_streams([s for s, _ in live], [c for _, c in live])
        if partial:
            r = _lib.partial_streams(streams)
            rows += sum(r.counters(i)[0] for i in range(len(streams)))
            calls += 1
            r.close()
        else:
            _lib.advance_streams(streams)
    out = _lib.finish_streams(streams)
    res = [(out.words(i), out.costs(i)) for i in range(len(pcms))]
    for s in streams:
        s.close()
    return res, rows, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["advance", "partial", "both"], default="both")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--round", type=int, default=16000, help="samples per stream and round (16000 = 1 s)")
    args = ap.parse_args()
    md, gd = configs.build_grammar_model(Path(tempfile.mkdtemp()) / "c4")
    model = _lib.Model(md, gd, _lib.default_opts(prune_output_pdfs=1))
    model.to_device()
    pcms = configs.stream_utterances(args.streams)
    modes = ["advance", "partial"] if args.mode == "both" else [args.mode]
    out = {"streams": args.streams, "round_samples": args.round, "steps": args.steps,
           "full_walk": os.environ.get("RS_PARTIAL_FULL_WALK", "0")}
    results = {}
    for mode in modes:
        for _ in range(args.warmup):
            step(model, pcms, args.round, mode == "partial")
        t = time.perf_counter()
        for _ in range(args.steps):
            res, rows, calls = step(model, pcms, args.round, mode == "partial")
        out[f"{mode}_ms_per_step"] = round(1e3 * (time.perf_counter() - t) / args.steps, 2)
        if mode == "partial":
            out["partial_calls_per_step"] = calls
            out["bp_rows_read_per_stream_and_call"] = round(rows / max(calls * args.streams, 1), 1)
        results[mode] = res
    if len(results) == 2:
        out["finish_identical"] = results["advance"] == results["partial"]
        out["added_step_time_pct"] = round(100.0 * (out["partial_ms_per_step"] / out["advance_ms_per_step"] - 1.0), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
