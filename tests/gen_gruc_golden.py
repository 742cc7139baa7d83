#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/gruc/<case>.npz for the cases of tests/gruc_cases.py (runs on the CPU, in the
build container, after build() has compiled the reference's binaries into oracle/_ref/bin).

Per case the REFERENCE decodes the case's clip with online2-wav-nnet3-latgen-faster (offline) and with
online2-cli-nnet3-decode-faster (streamed, 1024-sample ticks), the argv being oracle/gen_golden.py's, and rs-dump
(oracle/drivers/rs-dump.cc) dumps what the decodable saw.  Stored: exit status, 5-best text, graph and acoustic costs and frame
count of both modes; `input` (the network's input rows), the iVectors with their chunk ticks and the log-likelihoods, in full; the
network CollapseModel leaves (rs-dump collapsed) and the left / right context the looped decodable computed.  The rand() position
of the set-up is not stored: a recurrent compilation's draws are not replayed.  gc_dither_default has no golden: the script only
checks that the reference's set-up accepts the model.

Usage: python tests/gen_gruc_golden.py [case ...]
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
from oracle.gen_golden import BIN, decoder_args, parse_vec_ark, run  # noqa: E402
from tests import gruc_cases as lc  # noqa: E402


def dump(case: dict, mode: str, conf: Path, mdl: Path, wav: Path, out_dir: Path, env: dict, n_samples: int, has_iv: bool) -> dict:
    out_dir.mkdir()
    p = subprocess.run(["rs-dump", f"--config={conf}", "--acoustic-scale=1.0", mode, str(mdl), str(wav), str(out_dir)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError(f"rs-dump {mode} failed ({p.returncode}): {p.stderr[-400:]!r}")
    d = {k: np.load(out_dir / f"{k}.npy") for k in ("loglikes", "input") + (("ivector", "chunk_tick") if has_iv else ())}
    T = d["input"].shape[0]
    fsf = int(case.get("conf_opts", {}).get("frame-subsampling-factor", 1))
    assert T == (0 if n_samples < 400 else 1 + (n_samples - 400) // 160), (T, n_samples)
    assert d["loglikes"].shape[0] == (T + fsf - 1) // fsf and np.isfinite(d["loglikes"]).all() and np.isfinite(d["input"]).all()
    if has_iv:
        assert d["ivector"].shape[0] == d["chunk_tick"].shape[1] >= 1 and np.isfinite(d["ivector"]).all()
    m = re.search(rb"chunk (\d+), L (-?\d+), R (-?\d+)", p.stderr)
    d["context"] = np.array([int(m.group(2)), int(m.group(3))], np.int32)
    return d


def gen_case(name: str) -> None:
    case = lc.CASES[name]
    env = dict(os.environ, PATH=f"{BIN}:{os.environ['PATH']}")
    if name in lc.NO_GOLDEN:
        with tempfile.TemporaryDirectory() as td:
            model_dir = lc.build_case_files(name, Path(td))[0]
            rp = run(["rs-dump", f"--config={model_dir / 'model' / 'online' / 'conf' / 'online.conf'}", "randpos",
                      str(model_dir / "model" / "model" / "final.mdl"), "-", "-"], env=env)
            print(f"{name}: no golden; the reference's set-up accepts the model (rand position {int(rp.stdout)})")
        return
    has_iv = case["spec"].get("ivector_dim", 1) > 0
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        model_dir, graph_dir, wav, pcm = lc.build_case_files(name, root)
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
            sh = (f"lattice-to-nbest --n={lc.NBEST} --acoustic-scale=1.0 ark:{lat} ark:- | "
                  f"nbest-to-linear ark:- ark:/dev/null ark,t:- ark,t:{root}/lm.txt ark,t:{root}/ac.txt")
            q = run(["bash", "-c", sh], env=env)
            out[f"{mode}_nbest_text"] = np.frombuffer(q.stdout, dtype=np.uint8)
            lm = parse_vec_ark((root / "lm.txt").read_text())
            ac = parse_vec_ark((root / "ac.txt").read_text())
            keys = sorted(lm, key=lambda k: int(k.split("-")[1]))
            out[f"{mode}_graph_cost"] = np.array([lm[k][0] for k in keys], np.float32)
            out[f"{mode}_acoustic_cost"] = np.array([ac[k][0] for k in keys], np.float32)
            d = dump(case, mode, conf, mdl, wav, root / f"dump_{mode}", env, len(pcm), has_iv)
            out[f"{mode}_num_frames"] = np.int32(d["loglikes"].shape[0])
            out[f"{mode}_loglikes"] = d["loglikes"]
            if mode == "offline":
                out["input"] = d["input"]
                out["context"] = d["context"]
            if has_iv:
                out[f"{mode}_ivector"] = d["ivector"][:1] if mode == "offline" else d["ivector"]
                out[f"{mode}_chunk_tick"] = d["chunk_tick"][0].astype(np.int32)
        cl = run(["rs-dump", f"--config={conf}", "collapsed", str(mdl), "-", "-"], env=env)
        out["collapsed"] = np.frombuffer(cl.stdout, dtype=np.uint8)
        out["case_json"] = np.frombuffer(json.dumps(case, sort_keys=True).encode(), dtype=np.uint8)
        lc.GOLDEN.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(lc.GOLDEN / f"{name}.npz", **out)
        txt = bytes(out.get("offline_nbest_text", np.zeros(0, np.uint8))).decode().strip().replace("\n", " | ")
        rng = f" |input| <= {np.abs(out['input']).max():.4g} |loglike| <= {np.abs(out['offline_loglikes']).max():.4g}" if "input" in out else ""
        gaps = ""
        for mode in ("offline", "stream"):
            if f"{mode}_graph_cost" in out:
                tot = out[f"{mode}_graph_cost"] + out[f"{mode}_acoustic_cost"]
                gaps += f" {mode} min n-best gap {np.diff(tot).min() if len(tot) > 1 else float('inf'):.3g}"
        print(f"{name}: status {int(out['offline_status'])}/{int(out['stream_status'])} T={int(out.get('offline_num_frames', -1))}{rng}{gaps} offline: {txt}")


if __name__ == "__main__":
    for n in sys.argv[1:] or list(lc.CASES):
        gen_case(n)
