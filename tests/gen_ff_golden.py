#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/ff/<case>.npz for the cases of tests/ff_cases.py (runs on the CPU, in the build
container, after build() has compiled the reference's binaries into oracle/_ref/bin).

Per case the REFERENCE decodes the case's clip with online2-wav-nnet3-latgen-faster (offline) and with
online2-cli-nnet3-decode-faster (streamed, 1024-sample ticks), the argv being oracle/gen_golden.py's, and rs-dump
(oracle/drivers/rs-dump.cc) dumps what the decodable saw.  Stored: exit status, 5-best text, graph and acoustic costs and frame
count of both modes; `input` (the network's input rows), the iVectors with their chunk ticks and the log-likelihoods, in full; the
network CollapseModel leaves (rs-dump collapsed) and the left / right context the looped decodable computed.

The script ends with an error where adjacent n-best hypotheses of a case are closer than 0.02 in total cost (ten times the GPU
tests' cost tolerance): such a case gets another audio seed in the table, never a looser margin.

Usage: python tests/gen_ff_golden.py [case ...]
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle.gen_golden import BIN, decoder_args, parse_vec_ark, run  # noqa: E402
from tests import ff_cases as ff  # noqa: E402
from tests.gen_lstm_golden import dump  # noqa: E402

MIN_GAP = 0.02


def gen_case(name: str) -> float:
    """Writes the case's golden; returns the smallest gap between adjacent n-best hypotheses of either mode."""
    case = ff.CASES[name]
    env = dict(os.environ, PATH=f"{BIN}:{os.environ['PATH']}")
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        model_dir, graph_dir, wav, pcm = ff.build_case_files(name, root)
        conf = model_dir / "model" / "online" / "conf" / "online.conf"
        mdl = model_dir / "model" / "model" / "final.mdl"
        out = {}
        for mode in ("offline", "stream"):
            lat = root / f"{mode}.lat"
            if mode == "offline":
                cmd = ["online2-wav-nnet3-latgen-faster", "--online=false", "--do-endpointing=false",
                       f"--word-symbol-table={graph_dir / 'words.txt'}", f"--config={conf}", *decoder_args(case),
                       str(mdl), str(graph_dir / "HCLG.fst"), "ark:echo utt utt|", f"scp:echo utt {wav}|", f"ark:{lat}"]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            else:
                cmd = ["online2-cli-nnet3-decode-faster", f"--config={conf}", *decoder_args(case), str(mdl),
                       str(graph_dir / "HCLG.fst"), str(graph_dir / "words.txt"), f"ark:{lat}"]
                p = subprocess.run(cmd, env=env, input=pcm.astype("<i2").tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            out[f"{mode}_status"] = np.int32(p.returncode)
            if p.returncode != 0:
                out[f"{mode}_stderr"] = np.frombuffer(p.stderr[-400:], dtype=np.uint8)
                continue
            sh = (f"lattice-to-nbest --n={ff.NBEST} --acoustic-scale=1.0 ark:{lat} ark:- | "
                  f"nbest-to-linear ark:- ark:/dev/null ark,t:- ark,t:{root}/lm.txt ark,t:{root}/ac.txt")
            q = run(["bash", "-c", sh], env=env)
            out[f"{mode}_nbest_text"] = np.frombuffer(q.stdout, dtype=np.uint8)
            lm = parse_vec_ark((root / "lm.txt").read_text())
            ac = parse_vec_ark((root / "ac.txt").read_text())
            keys = sorted(lm, key=lambda k: int(k.split("-")[1]))
            out[f"{mode}_graph_cost"] = np.array([lm[k][0] for k in keys], np.float32)
            out[f"{mode}_acoustic_cost"] = np.array([ac[k][0] for k in keys], np.float32)
            d = dump(case, mode, conf, mdl, wav, root / f"dump_{mode}", env, len(pcm), True)
            out[f"{mode}_num_frames"] = np.int32(d["loglikes"].shape[0])
            out[f"{mode}_loglikes"] = d["loglikes"]
            if mode == "offline":
                out["input"] = d["input"]
                out["context"] = d["context"]
            out[f"{mode}_ivector"] = d["ivector"][:1] if mode == "offline" else d["ivector"]
            out[f"{mode}_chunk_tick"] = d["chunk_tick"][0].astype(np.int32)
        cl = run(["rs-dump", f"--config={conf}", "collapsed", str(mdl), "-", "-"], env=env)
        out["collapsed"] = np.frombuffer(cl.stdout, dtype=np.uint8)
        out["case_json"] = np.frombuffer(json.dumps(case, sort_keys=True).encode(), dtype=np.uint8)
        ff.GOLDEN.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(ff.GOLDEN / f"{name}.npz", **out)
        txt = bytes(out.get("offline_nbest_text", np.zeros(0, np.uint8))).decode().strip().replace("\n", " | ")
        rng = f" |input| <= {np.abs(out['input']).max():.4g} |loglike| <= {np.abs(out['offline_loglikes']).max():.4g}" if "input" in out else ""
        gaps, worst = "", float("inf")
        for mode in ("offline", "stream"):
            if f"{mode}_graph_cost" in out:
                tot = out[f"{mode}_graph_cost"].astype(np.float64) + out[f"{mode}_acoustic_cost"]
                gap = float(np.diff(tot).min()) if len(tot) > 1 else float("inf")
                worst = min(worst, gap)
                gaps += f" {mode} min n-best gap {gap:.3g}"
            else:
                gaps += f" {mode}: {bytes(out[f'{mode}_stderr'])[-160:]!r}"
        print(f"{name}: status {int(out['offline_status'])}/{int(out['stream_status'])} T={int(out.get('offline_num_frames', -1))}{rng}{gaps} offline: {txt}")
        return worst


if __name__ == "__main__":
    close = [(n, gap) for n in (sys.argv[1:] or list(ff.CASES)) for gap in [gen_case(n)] if gap <= MIN_GAP]
    if close:
        sys.exit(f"n-best hypotheses closer than {MIN_GAP}: {close}; give these cases another audio seed")
