#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden generator for the endpoint-detection tests (runs where oracle/_ref exists).

Per case of tests/endpoint_cases.py it runs the reference's online2-wav-nnet3-latgen-faster with --online=true --do-endpointing=true
--chunk-length=0.064 (1024 samples at 16 kHz: per chunk what the stream binary does per tick; it breaks out of its chunk loop when
EndpointDetected says so, online2-wav-nnet3-latgen-faster.cc:270-274) and records, as data only, under tests/golden/endpoint/<case>.json:
  frames        the frames of the lattice it wrote = NumFramesDecoded() at the break (the log's "over N frames")
  stopped_early whether it broke before the last chunk
  rule, values  the --verbose=2 line of RuleActivated: which rule, contains_nonsilence, trailing_silence, relative_cost, utterance_length
  nbest         lattice-to-nbest | nbest-to-linear: words and (graph, acoustic) costs per hypothesis
  lines         the --endpoint.* lines used
and checks the conditions the tests rely on with the CPU oracle (tests/endpoint_cases.py: TickOracle) on every tick before the break:
no rule fires earlier, and on the deciding tick and all earlier ones every comparison a rule makes is clear of its threshold (one
frame on the two durations, 100 x the partial tests' cost tolerance on the relative cost), so that a rounding difference cannot move
the decision.  A case that fails a check is reported and must be replaced.

Usage: python tools/gen_endpoint_golden.py [--explore] [case ...]
  --explore: no reference run; prints per tick what the oracle sees (frames, the best path's last phone runs, relative cost) -- used
             to choose silence lists and thresholds for new cases.
"""
from __future__ import annotations

import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle import pipeline  # noqa: E402
from oracle.gen_golden import decoder_args, parse_vec_ark  # noqa: E402
from tests import cases, endpoint_cases as ec  # noqa: E402

BIN = REPO / "oracle" / "_ref" / "bin"
COST_ATOL, COST_RTOL = 1e-4, 2e-6          # tests/test_gpu_stream_partial.py
RULE_KEYS = ("must-contain-nonsilence", "min-trailing-silence", "max-relative-cost", "min-utterance-length")
DEFAULT_RULES = [(False, 5.0, np.inf, 0.0), (True, 0.5, 2.0, 0.0), (True, 1.0, 8.0, 0.0), (True, 2.0, np.inf, 0.0), (False, 0.0, np.inf, 20.0)]


def rules_of(case: dict):
    rules = [list(r) for r in DEFAULT_RULES]
    for k, v in case["lines"].items():
        m = re.fullmatch(r"rule([1-5])\.(.+)", k)
        if m:
            i = RULE_KEYS.index(m.group(2))
            rules[int(m.group(1)) - 1][i] = (str(v).lower() in ("true", "1", "t")) if i == 0 else float(v)
    return rules


def silence_of(case: dict):
    return [int(p) for p in str(case["lines"]["silence-phones"]).split(":")]


def fired(rules, frames, sil, shift, cost):
    f32 = np.float32
    ul, ts = f32(frames) * f32(shift), f32(sil) * f32(shift)
    for k, (must, min_sil, max_cost, min_len) in enumerate(rules):
        if ((ul > ts) or not must) and ts >= f32(min_sil) and f32(cost) <= f32(max_cost) and ul >= f32(min_len):
            return k + 1
    return 0


def clearance_problems(rules, frames, sil, shift, cost):
    """Comparisons of any rule that sit within the agreed distance of their threshold.  (contains_nonsilence, utterance_length >
    trailing_silence, compares two frame counts times the same shift: no cost enters it, so it has no clearance to keep.)"""
    out = []
    ul, ts = frames * shift, sil * shift
    tol = 100.0 * (COST_ATOL + COST_RTOL * abs(cost)) if np.isfinite(cost) else 0.0
    for k, (must, min_sil, max_cost, min_len) in enumerate(rules):
        if abs(ts - min_sil) < shift and min_sil > 0 and abs(ts - min_sil) > 1e-9:
            out.append(f"rule{k + 1}: trailing silence {ts:.3f} within a frame of {min_sil}")
        if abs(ts - min_sil) <= 1e-9 and min_sil > 0:
            out.append(f"rule{k + 1}: trailing silence {ts:.3f} exactly at {min_sil}")
        if np.isfinite(max_cost) and np.isfinite(cost) and abs(cost - max_cost) < tol:
            out.append(f"rule{k + 1}: relative cost {cost:.5f} within {tol:.4f} of {max_cost}")
        if min_len > 0 and abs(ul - min_len) < shift:
            out.append(f"rule{k + 1}: utterance length {ul:.3f} within a frame of {min_len}")
    return out


def oracle_ticks(name: str, root: Path):
    """-> (files, per tick (frames, trailing silence, relative cost, margin)), phones function"""
    case = ec.ENDPOINT_CASES[name]
    base = cases.CASES[case["base"]]
    model_dir, graph_dir, wav, pcm = ec.build_files(name, root)
    orc = pipeline.Oracle(model_dir, graph_dir, **base.get("opts", {}))
    feats = orc.features(pcm)
    _, _, ll = orc.loglikes_stream(feats, len(pcm))
    ll = np.ascontiguousarray(ll[::orc.fsf])
    tick = ec.TickOracle(orc, ec.tid_to_phone(cases.case_spec(base)))
    frames = ec.frames_after_ticks(orc, len(pcm))
    shift = ec.frame_shift(orc)
    return (model_dir, graph_dir, wav, pcm), orc, ll, tick, frames, shift


def explore(name: str) -> None:
    with tempfile.TemporaryDirectory() as td:
        _, orc, ll, tick, frames, shift = oracle_ticks(name, Path(td))
        print(f"== {name}: {len(frames)} complete ticks, frame shift {shift}, chunk {orc.chunk}, fsf {orc.fsf}")
        seen = -1
        for j, n in enumerate(frames):
            if n == seen or n == 0:
                continue
            seen = n
            ph = tick.best_phones(ll, n)
            runs = []
            for p in ph:
                if runs and runs[-1][0] == p:
                    runs[-1][1] += 1
                else:
                    runs.append([p, 1])
            _, rel, margin = tick.values(ll, n, [])
            print(f"tick {j:3d} frames {n:4d} rel {rel:9.4f} margin {margin:8.4f} last runs (phone x frames, newest first): "
                  + " ".join(f"{p}x{c}" for p, c in runs[:8]))


def gen(name: str) -> bool:
    case = ec.ENDPOINT_CASES[name]
    base = cases.CASES[case["base"]]
    env = dict(os.environ, PATH=f"{BIN}:{os.environ['PATH']}")
    ok = True
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        (model_dir, graph_dir, wav, pcm), orc, ll, tick, frames, shift = oracle_ticks(name, root)
        conf = model_dir / "model" / "online" / "conf" / "online.conf"
        mdl = model_dir / "model" / "model" / "final.mdl"
        lat = root / "endpoint.lat"
        cmd = ["online2-wav-nnet3-latgen-faster", "--online=true", "--do-endpointing=true", "--chunk-length=0.064", "--verbose=2",
               f"--word-symbol-table={graph_dir / 'words.txt'}", f"--config={conf}", *decoder_args(base),
               str(mdl), str(graph_dir / "HCLG.fst"), "ark:echo utt utt|", f"scp:echo utt {wav}|", f"ark:{lat}"]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        log = p.stderr.decode()
        m = re.search(r"over (\d+) frames", log)
        ref_frames = int(m.group(1))
        act = re.search(r"Endpointing rule (rule\d) activated: (true|false),([^,]+),([^,]+),([^\s,]+)", log)
        sh = (f"lattice-to-nbest --n={cases.NBEST} --acoustic-scale=1.0 ark:{lat} ark:- | "
              f"nbest-to-linear ark:- ark:/dev/null ark,t:- ark,t:{root}/lm.txt ark,t:{root}/ac.txt")
        q = subprocess.run(["bash", "-c", sh], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        lm, ac = parse_vec_ark((root / "lm.txt").read_text()), parse_vec_ark((root / "ac.txt").read_text())
        keys = sorted(lm, key=lambda k: int(k.split("-")[1]))
        words = {l.split()[0]: [int(w) for w in l.split()[1:]] for l in q.stdout.decode().splitlines() if l.strip()}
        nbest = [dict(words=words[k], graph_cost=lm[k][0], acoustic_cost=ac[k][0]) for k in keys]
        # ---- where did it stop?  before the last chunk <=> a rule was activated on a tick whose frames the oracle's schedule gives
        n_chunks = (len(pcm) + ec.TICK - 1) // ec.TICK
        rules, sil = rules_of(case), silence_of(case)
        stop_tick = None
        if act is not None:
            cands = [j for j, n in enumerate(frames) if n == ref_frames]
            stop_tick = cands[0] if cands else None
        stopped_early = act is not None and stop_tick is not None and stop_tick < n_chunks - 1
        if act is not None and stop_tick is None:
            # the rule fired on the last chunk, after InputFinished(): not an early stop, the tail is the wav binary's own
            stopped_early = False
        # ---- the oracle's view of every tick up to the stop (all complete ticks before the last chunk when it never stops)
        upto = stop_tick if stopped_early else min(len(frames), n_chunks - 1) - 1
        last_n, problems = -1, []
        for j in range(upto + 1):
            n = frames[j]
            if n == 0 or n == last_n:
                continue
            last_n = n
            ts, rel, margin = tick.values(ll, n, sil)
            f = fired(rules, n, ts, shift, rel)
            deciding = stopped_early and j == stop_tick
            if not deciding and f:
                problems.append(f"tick {j} ({n} frames): the oracle fires rule{f} before the reference stops")
            if deciding:
                if f != int(act.group(1)[4:]):
                    problems.append(f"tick {j}: the oracle fires rule{f}, the reference {act.group(1)}")
                ref_ts, ref_rel, ref_ul = float(act.group(3)), float(act.group(4)), float(act.group(5))
                if abs(ref_ts - ts * shift) > 1e-4 or abs(ref_ul - n * shift) > 1e-4:
                    problems.append(f"tick {j}: durations differ: oracle {ts * shift} / {n * shift}, reference {ref_ts} / {ref_ul}")
                if np.isfinite(rel) != np.isfinite(ref_rel) or (np.isfinite(rel) and abs(rel - ref_rel) > 1e-2):
                    problems.append(f"tick {j}: relative cost differs: oracle {rel}, reference {ref_rel}")
            if margin < 100.0 * COST_ATOL:
                problems.append(f"tick {j} ({n} frames): the two best frontier tokens are {margin:.2e} apart")
            problems += [f"tick {j} ({n} frames): " + s for s in clearance_problems(rules, n, ts, shift, rel)]
        for s in problems:
            print(f"  !! {name}: {s}")
        ok = not problems
        out = dict(case=name, base=case["base"], tail=case["tail"], lines=ec.endpoint_lines(case), frames=ref_frames,
                   stopped_early=bool(stopped_early), stop_tick=stop_tick if stopped_early else None,
                   rule=int(act.group(1)[4:]) if stopped_early else 0,
                   values=dict(contains_nonsilence=act.group(2) == "true", trailing_silence=float(act.group(3)),
                               relative_cost=float(act.group(4)) if act.group(4) != "inf" else "inf",
                               utterance_length=float(act.group(5))) if stopped_early else None,
                   num_chunks=n_chunks, nbest=nbest)
        ec.GOLDEN_DIR.mkdir(parents=True, exist_ok=True)
        (ec.GOLDEN_DIR / f"{name}.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
        print(f"{name}: frames {ref_frames} stopped_early {stopped_early} tick {stop_tick} rule {out['rule']} "
              f"values {out['values']} best {nbest[0]['words'] if nbest else None}{'' if ok else '   <-- NOT CLEAR'}")
    return ok


def main() -> None:
    args = sys.argv[1:]
    exploring = "--explore" in args
    names = [a for a in args if not a.startswith("--")] or list(ec.ENDPOINT_CASES)
    if exploring:
        for n in names:
            explore(n)
        return
    results = {n: gen(n) for n in names}
    if names == list(ec.ENDPOINT_CASES):
        g = [ec.load_golden(n) for n in names]
        early = [x for x in g if x["stopped_early"]]
        rules = {x["rule"] for x in early}
        finite = [x for x in early if np.isfinite(rules_of(ec.ENDPOINT_CASES[x["case"]])[x["rule"] - 1][2])]
        print(f"{len(early)} cases stop early over rules {sorted(rules)} ({len(finite)} by a rule with a finite max-relative-cost); "
              f"{len(g) - len(early)} never stop")
        assert len(early) >= 8 and len(rules) >= 3 and finite and len(g) - len(early) >= 2, "the set of cases misses the conditions"
    assert all(results.values()), [n for n, ok in results.items() if not ok]


if __name__ == "__main__":
    main()
