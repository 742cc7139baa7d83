"""What an endpoint query costs beside a partial result on the streams workload: 64 concurrent 30 s streams (bench.py's `streams`
audio and model) fed TICK BY TICK (1024 samples per stream and round), each round followed by ONE call over all 64 streams:
  --mode endpoint   rs_streams_endpoint
  --mode partial    rs_streams_partial              (the yardstick: the parent commit has it)
  --mode split      rs_streams_endpoint twice: the second call finds no new tick, so it is the query without the catch-up
Per mode a warm-up step, then --reps rounds in which the modes alternate; per step the time spent inside the calls is summed and divided by the number of calls.
Prints one JSON line: median and range over the repetitions of the microseconds per call, the catch-up share of an endpoint call
(1 - second call / first call, from --mode split), and the back-pointer rows read per stream and call.
usage (GPU box): python profiles/micro/endpoint_cost.py
       rocprofv3 --kernel-trace --stats -d <dir> -o endpoint -- python profiles/micro/endpoint_cost.py --mode endpoint --reps 1"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rhasspy_speech_amd import _lib  # noqa: E402
from tests import configs  # noqa: E402

TICK = 1024


def step(model, pcms, mode, opts):
    streams = [_lib.Stream(model) for _ in pcms]
    t_first = t_second = 0.0
    calls = rows = detected = 0
    for k in range(0, max(len(p) for p in pcms) // TICK * TICK, TICK):
        live = [(s, p[k:k + TICK]) for s, p in zip(streams, pcms) if k + TICK <= len(p)]
        _lib.accept_streams([s for s, _ in live], [c for _, c in live])
        t0 = time.perf_counter()
        if mode == "partial":
            r = _lib.partial_streams(streams)
            t_first += time.perf_counter() - t0
            rows += sum(r.counters(i)[0] for i in range(len(streams)))
            r.close()
        else:
            recs = _lib.endpoint_streams(streams, opts)
            t1 = time.perf_counter()
            t_first += t1 - t0
            if mode == "split":
                _lib.endpoint_streams(streams, opts)
                t_second += time.perf_counter() - t1
            rows += sum(x.rows_read for x in recs)
            detected += sum(1 for x in recs if x.detected)
        calls += 1
    for s in streams:
        s.close()
    return 1e6 * t_first / calls, 1e6 * t_second / calls, rows / (calls * len(pcms)), detected


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["endpoint", "partial", "split", "all"], default="all")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--silence-phones", default=None, help="default: the model's online.conf")
    args = ap.parse_args()
    md, gd = configs.build_grammar_model(Path(tempfile.mkdtemp()) / "c4")
    model = _lib.Model(md, gd, _lib.default_opts(prune_output_pdfs=1))
    model.to_device()
    opts = model.endpoint_opts()
    if args.silence_phones:
        opts.silence_phones = args.silence_phones.encode()
    pcms = configs.stream_utterances(args.streams)
    out = {"streams": args.streams, "ticks_per_step": max(len(p) for p in pcms) // TICK, "reps": args.reps,
           "silence_phones": opts.silence_phones.decode()}
    modes = ["partial", "endpoint", "split"] if args.mode == "all" else [args.mode]
    for mode in modes:
        for _ in range(args.warmup):
            step(model, pcms, mode, opts)
    runs = {mode: [] for mode in modes}
    for _ in range(args.reps):          # the modes alternate: whatever else the machine does meets all of them alike
        for mode in modes:
            runs[mode].append(step(model, pcms, mode, opts))
    for mode in modes:
        first = [r[0] for r in runs[mode]]
        out[f"{mode}_us_per_call_median"] = round(statistics.median(first), 1)
        out[f"{mode}_us_per_call_range"] = [round(min(first), 1), round(max(first), 1)]
        out[f"{mode}_rows_read_per_stream_and_call"] = round(runs[mode][-1][2], 1)
        if mode == "split":
            second = [r[1] for r in runs[mode]]
            out["query_only_us_per_call_median"] = round(statistics.median(second), 1)
            out["query_only_us_per_call_range"] = [round(min(second), 1), round(max(second), 1)]
            out["catch_up_share_of_an_endpoint_call"] = round(1.0 - statistics.median(second) / statistics.median(first), 3)
        if mode != "partial":
            out[f"{mode}_detections"] = runs[mode][-1][3]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
