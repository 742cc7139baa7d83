"""What the decode contexts' arenas do while the headline run warms up and while it is timed: the headline model and batch
(tests/configs.py), one call alone, then four calls in flight, then 20 steps with four in flight -- the order of bench.py's
run_steps with `--steps 20 --warmup 5`, the first calls of a phase started 0.6 ms apart like there.  Prints the `arenas:` line of
rs_model_describe after each phase and every call's wall time (a call that allocates, or that runs beside one that does, shows).

    python profiles/micro/cold_contexts.py [--steps 20] [--inflight 4] [--utts 256]
"""
import argparse
import concurrent.futures
import os
import re
import sys
import tempfile
import time
from pathlib import Path

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # (bench.py does the same)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))

from rhasspy_speech_amd import _lib      # noqa: E402
from tests import configs                # noqa: E402


def arenas_line(model):
    return re.search(r"^arenas: .*$", model.describe(), re.M).group(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--stagger-ms", type=float, default=0.6)
    args = ap.parse_args()
    work = tempfile.TemporaryDirectory(prefix="rs_cold_")
    model_dir, graph_dir = configs.build_grammar_model(Path(work.name) / "grammar")
    pcms = configs.grammar_utterances(args.utts)
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(prune_output_pdfs=1))
    model.to_device()
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=args.inflight)
    first = []

    def phase(name, n):
        t_start = time.perf_counter()

        def call(delay=0.0):
            if delay > 0:
                time.sleep(delay)
            t_in = time.perf_counter()
            res = model.decode_batch(pcms)
            return res, (t_in - t_start) * 1e3, (time.perf_counter() - t_start) * 1e3
        futures = [pool.submit(call, i * args.stagger_ms * 1e-3) for i in range(min(n, args.inflight))]
        walls = []
        for k in range(n):
            res, t_in, t_out = futures[k].result()
            if len(futures) < n:
                futures.append(pool.submit(call))
            words = [res.words(u) for u in range(len(pcms))]
            if not first:
                first.append(words)
            if words != first[0]:
                raise SystemExit(f"cold_contexts.py: {name}, call {k}: transcripts differ from the first call's")
            walls.append((t_in, t_out))
        total = (time.perf_counter() - t_start) * 1e3
        print(f"{name}: {n} calls in {total:.2f} ms ({total / n:.3f} ms per call)")
        print("  call wall times, ms (entered -> returned): " + "  ".join(f"{b - a:.2f} ({a:.1f}->{b:.1f})" for a, b in walls))
        line = arenas_line(model)
        print("  " + line, flush=True)
        return line

    phase("alone", 1)
    before = phase(f"warm-up, {args.inflight} in flight", args.inflight)
    after = phase(f"{args.steps} steps, {args.inflight} in flight", args.steps)
    print("arenas over the timed steps: " + ("unchanged" if after == before else "CHANGED"))
    m = re.search(r"device blocks=(\d+) bytes=(\d+) allocations=(\d+)", after)
    print(f"resident device arena memory: {int(m.group(2)) / 1e9:.3f} GB in {m.group(1)} blocks after {m.group(3)} allocations")


if __name__ == "__main__":
    main()
