#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden generator for the speaker-adaptation tests (runs where oracle/_ref exists).

Per case of tests/adaptation_cases.py it runs the reference's online2-wav-nnet3-latgen-faster ONCE with --online=true
--chunk-length=0.064 (1024 samples at 16 kHz: per chunk what the stream binary does per tick) and a spk2utt line "spk u1 u2 [u3]", so
that the binary itself carries the adaptation state from utterance to utterance (online2-wav-nnet3-latgen-faster.cc:203-205,
220-221, 287-288), and records, as data only, under tests/golden/adaptation/<case>.json per utterance:
  frames   the frames of the lattice it wrote (the log's "over N frames")
  nbest    lattice-to-nbest | nbest-to-linear: words and (graph, acoustic) costs of the 5 best hypotheses
and the same with every utterance as its own speaker ("fresh").  The case with --endpoint.* lines runs with --do-endpointing=true.
Two conditions are enforced; a case that fails one is reported and must be replaced:
  (a) on every utterance after the first, the adapted best path's acoustic cost differs from the fresh one by at least 100 x the
      tests' cost tolerance -- otherwise the case cannot tell the feature from its absence;
  (b) tests/adaptation_cases.py's AdaptedOracle gives the reference's 5-best lists, with costs within the tolerance at which
      tests/test_oracle_golden.py pins the oracle;
  (c) ... and within the tighter tolerance the GPU tests hold the device to: an utterance on which the sequential double-precision
      oracle is further from the reference than that cannot pin the device to the reference;
  (d) no utterance's last read completes a nnet chunk (tests/adaptation_cases.py: last_read_completes_a_chunk): there this binary,
      which finishes its input before the last chunk is decoded, and the stream binary, which the streams restate, give the chunk
      different iVectors.

Usage: python tools/gen_adaptation_golden.py [case ...]
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
from tests import adaptation_cases as ac, cases  # noqa: E402

BIN = REPO / "oracle" / "_ref" / "bin"
COST_ATOL, COST_RTOL = 1e-4, 2e-6                # tests/test_gpu_stream_adaptation.py
ORACLE_RTOL, ORACLE_ATOL = 2e-4, 2e-3            # tests/test_oracle_golden.py


def run_reference(root: Path, tag: str, spk2utt: str, model_dir: Path, graph_dir: Path, wavs, endpointing: bool, env) -> dict:
    """-> {utterance: dict(frames, nbest)}"""
    conf = model_dir / "model" / "online" / "conf" / "online.conf"
    mdl = model_dir / "model" / "model" / "final.mdl"
    lat, s2u, scp = root / f"{tag}.lat", root / f"{tag}.spk2utt", root / f"{tag}.scp"
    s2u.write_text(spk2utt)
    scp.write_text("".join(f"u{i + 1} {w}\n" for i, w in enumerate(wavs)))
    cmd = ["online2-wav-nnet3-latgen-faster", "--online=true", "--chunk-length=0.064", "--verbose=2", f"--do-endpointing={'true' if endpointing else 'false'}",
           f"--word-symbol-table={graph_dir / 'words.txt'}", f"--config={conf}", *decoder_args({}),
           str(mdl), str(graph_dir / "HCLG.fst"), f"ark:{s2u}", f"scp:{scp}", f"ark:{lat}"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    frames = {m.group(1): int(m.group(2)) for m in re.finditer(r"for utterance (\S+) is \S+ over (\d+) frames", p.stderr.decode())}
    sh = (f"lattice-to-nbest --n={cases.NBEST} --acoustic-scale=1.0 ark:{lat} ark:- | "
          f"nbest-to-linear ark:- ark:/dev/null ark,t:- ark,t:{root}/{tag}.lm ark,t:{root}/{tag}.ac")
    q = subprocess.run(["bash", "-c", sh], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    lm, acw = parse_vec_ark((root / f"{tag}.lm").read_text()), parse_vec_ark((root / f"{tag}.ac").read_text())
    words = {l.split()[0]: [int(w) for w in l.split()[1:]] for l in q.stdout.decode().splitlines() if l.strip()}
    out = {}
    for i in range(len(wavs)):
        u = f"u{i + 1}"
        keys = sorted((k for k in lm if k.rsplit("-", 1)[0] == u), key=lambda k: int(k.rsplit("-", 1)[1]))
        out[u] = dict(frames=frames[u], nbest=[dict(words=words[k], graph_cost=lm[k][0], acoustic_cost=acw[k][0]) for k in keys])
    return out


def stop_tick_of(orc, n_samples: int, frames: int):
    """The tick after which the reference stopped, from the frames it decoded: None = it read the whole utterance."""
    from tests import endpoint_cases as ec
    full = (orc.mfcc.num_frames(n_samples) + orc.fsf - 1) // orc.fsf
    if frames == full:
        return None
    per_tick = ec.frames_after_ticks(orc, n_samples)
    return per_tick.index(frames)


def gen(name: str) -> bool:
    case = ac.ADAPT_CASES[name]
    env = dict(os.environ, PATH=f"{BIN}:{os.environ['PATH']}")
    problems = []
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        model_dir, graph_dir, wavs, pcms = ac.build_files(name, root)
        utts = [f"u{i + 1}" for i in range(len(wavs))]
        endpointing = bool(case["endpoint"])
        adapted = run_reference(root, "adapted", "spk " + " ".join(utts) + "\n", model_dir, graph_dir, wavs, endpointing, env)
        fresh = run_reference(root, "fresh", "".join(f"s{u} {u}\n" for u in utts), model_dir, graph_dir, wavs, endpointing, env)
        orc = pipeline.Oracle(model_dir, graph_dir)
        ao = ac.AdaptedOracle(orc, model_dir)
        state = ao.fresh()
        stops = []
        for i, u in enumerate(utts):
            g = adapted[u]
            stop = stop_tick_of(orc, len(pcms[i]), g["frames"])
            stops.append(stop)
            if endpointing and (stop is not None) != (i == 0):
                problems.append(f"{u}: the reference {'stopped early' if stop is not None else 'did not stop'}; only utterance 1 is meant to stop")
            if stop is not None:
                # the clearance the endpoint generator asks of a length rule: a frame on either side of the threshold, on the deciding
                # tick and on the one before it
                from tests import endpoint_cases as ec
                shift, thr = ec.frame_shift(orc), float(case["endpoint"]["rule5.min-utterance-length"])
                per_tick = ec.frames_after_ticks(orc, len(pcms[i]))
                before = max([n for n in per_tick[:stop] if n != per_tick[stop]] or [0])
                if not (per_tick[stop] * shift - thr > shift and thr - before * shift > shift):
                    problems.append(f"{u}: utterance lengths {before * shift:.3f} / {per_tick[stop] * shift:.3f} are within a frame of {thr}")
            if stop is None and ac.last_read_completes_a_chunk(orc, len(pcms[i])):
                problems.append(f"{u}: its last read completes a nnet chunk: the wav binary and the stream binary differ there ({len(pcms[i])} samples)")
            if i > 0:
                a, f = g["nbest"][0]["acoustic_cost"], fresh[u]["nbest"][0]["acoustic_cost"]
                need = 100.0 * (COST_ATOL + COST_RTOL * abs(f))
                if abs(a - f) < need:
                    problems.append(f"{u}: adapted and fresh acoustic costs {a} / {f} are closer than {need:.4f}")
            tr, state = ao.run(pcms[i], state, stop_tick=stop, nbest=cases.NBEST)
            if tr.num_frames != g["frames"]:
                problems.append(f"{u}: the oracle decodes {tr.num_frames} frames, the reference {g['frames']}")
            if [p.words for p in tr.nbest] != [h["words"] for h in g["nbest"]]:
                problems.append(f"{u}: the oracle's {cases.NBEST}-best lists differ from the reference's")
            else:
                for what in ("graph_cost", "acoustic_cost"):
                    o, r = np.array([getattr(p, what) for p in tr.nbest]), np.array([h[what] for h in g["nbest"]])
                    if not np.allclose(o, r, rtol=ORACLE_RTOL, atol=ORACLE_ATOL):
                        problems.append(f"{u}: the oracle's {what} {o} vs the reference's {r}")
                    elif not np.allclose(o, r, rtol=COST_RTOL, atol=COST_ATOL + 5e-5):      # (+ the 4 decimals the reference's tools print)
                        # (c) the sequential CPU oracle itself is further from the reference than the GPU tests allow the device to be
                        problems.append(f"{u}: the oracle's {what} {o} is not within the GPU tests' tolerance of {r}")
                print(f"  {name} {u}: frames {g['frames']} stop {stop} best {g['nbest'][0]['words']} ac {g['nbest'][0]['acoustic_cost']:.4f} "
                      f"(fresh {fresh[u]['nbest'][0]['acoustic_cost']:.4f}, oracle {tr.nbest[0].acoustic_cost:.4f})")
        out = dict(case=name, utts=[dict(seed=s, samples=n) for s, n in case["utts"]], stop_ticks=stops, adapted=[adapted[u] for u in utts],
                   fresh=[fresh[u] for u in utts])
        ac.GOLDEN_DIR.mkdir(parents=True, exist_ok=True)
        (ac.GOLDEN_DIR / f"{name}.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    for s in problems:
        print(f"  !! {name}: {s}")
    print(f"{name}: {'ok' if not problems else 'NOT USABLE'}")
    return not problems


def main() -> None:
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(ac.ADAPT_CASES)
    results = {n: gen(n) for n in names}
    assert all(results.values()), [n for n, ok in results.items() if not ok]


if __name__ == "__main__":
    main()
