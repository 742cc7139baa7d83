"""What speaker adaptation costs on the streams workload: 64 concurrent streams (bench.py's `streams` model, the first --seconds of
its audio), one utterance per stream and repetition:
  adaptation_us_per_call   rs_streams_adaptation over the 64 ended streams, one call
  open_plain / open_adapted_us_per_stream   rs_stream_open against rs_stream_open_adapted with the state of the utterance before
  advance_plain / advance_adapted_ms_per_step   the time inside the accept + advance + finish calls of a step of 64 plain streams
                           against 64 adapted ones: the price of the speaker term in the CMVN kernel (and of nothing else: the
                           estimator and everything behind it run the same launches on other numbers)
Plain and adapted steps alternate within a repetition.  Prints one JSON line: median and range over --reps repetitions.
usage (GPU box): python profiles/micro/adaptation_cost.py"""
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

ROUND = 16 * 1024      # samples handed over per stream and round (bench.py's streams workload: 16 ticks)


def step(model, pcms, states):
    """-> (us per open, ms inside accept / advance / finish, us of the adaptation call, the states after)"""
    t0 = time.perf_counter()
    streams = [_lib.Stream(model, adaptation=st) for st in states]
    t_open = time.perf_counter() - t0
    t_adv = 0.0
    for k in range(0, max(len(p) for p in pcms), ROUND):
        live = [(s, p[k:k + ROUND]) for s, p in zip(streams, pcms) if k < len(p)]
        t0 = time.perf_counter()
        _lib.accept_streams([s for s, _ in live], [c for _, c in live])
        _lib.advance_streams([s for s, _ in live])
        t_adv += time.perf_counter() - t0
    t0 = time.perf_counter()
    _lib.finish_streams(streams).close()
    t_adv += time.perf_counter() - t0
    t0 = time.perf_counter()
    after = _lib.adaptation_of_streams(streams)
    t_get = time.perf_counter() - t0
    for s in streams:
        s.close()
    return 1e6 * t_open / len(pcms), 1e3 * t_adv, 1e6 * t_get, after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    md, gd = configs.build_grammar_model(Path(tempfile.mkdtemp()) / "c4")
    model = _lib.Model(md, gd, _lib.default_opts(prune_output_pdfs=1))
    model.to_device()
    n = int(16000 * args.seconds)
    pcms = [p[:n] for p in configs.stream_utterances(args.streams)]
    plain = [None] * len(pcms)
    _, _, _, carried = step(model, pcms, plain)      # warm-up; its states open the adapted steps
    step(model, pcms, carried)
    runs = {"plain": [], "adapted": []}
    for _ in range(args.reps):
        runs["plain"].append(step(model, pcms, plain)[:3])
        runs["adapted"].append(step(model, pcms, carried)[:3])
    out = {"streams": args.streams, "seconds": args.seconds, "reps": args.reps}

    def put(key, values, digits=1):
        out[f"{key}_median"] = round(statistics.median(values), digits)
        out[f"{key}_range"] = [round(min(values), digits), round(max(values), digits)]

    put("adaptation_us_per_call", [r[2] for r in runs["plain"] + runs["adapted"]])
    put("open_plain_us_per_stream", [r[0] for r in runs["plain"]])
    put("open_adapted_us_per_stream", [r[0] for r in runs["adapted"]])
    put("advance_plain_ms_per_step", [r[1] for r in runs["plain"]], 3)
    put("advance_adapted_ms_per_step", [r[1] for r in runs["adapted"]], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
