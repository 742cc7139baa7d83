#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/rates/<case>.npz for the cases of tests/rate_cases.py (runs on the CPU, in the
build container, after build() has compiled the reference's binaries into oracle/_ref/bin).

Per case the REFERENCE decodes the case's clip with online2-wav-nnet3-latgen-faster (offline; the wav is written at the case's rate)
and with online2-cli-nnet3-decode-faster --samp-freq=<rate> (streamed, 1024-sample ticks of the raw samples), the argv otherwise
being oracle/gen_golden.py's, and rs-dump (oracle/drivers/rs-dump.cc) dumps what the offline decodable saw.  Stored: exit status,
5-best text, graph and acoustic costs and frame count of both modes; offline also `input` (the network's input rows), the iVector
and the log-likelihoods, in full; the rand() position of the model set-up.

rs-dump's stream mode hands AcceptWaveform 16000 whatever the model's rate is (rs-dump.cc:173), so there are no per-tick dumps of the
stream here: the stream binary's text, costs and frame count are what is stored.

rs-dump's offline mode with an iVector extractor: after it has written loglikes / input / ivector / chunk_tick it rebuilds the
extractor's branch on an OnlineMfcc to dump cmvn / lda / lda_norm (rs-dump.cc:198-221).  On a filterbank model that rebuild has the
wrong dimension and ends the program.  Those three files are not asked for here; for that one run a non-zero exit is accepted AFTER
the four files before it have been found complete, exactly as tests/gen_fbank_golden.py does.  Every other rs-dump run must exit 0.

Usage: python tests/gen_rate_golden.py [case ...]
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
from tests import rate_cases as rc  # noqa: E402


def dump_offline(name: str, conf: Path, mdl: Path, wav: Path, out_dir: Path, env: dict, n_samples: int, has_iv: bool, fbank: bool) -> dict:
    out_dir.mkdir()
    p = subprocess.run(["rs-dump", f"--config={conf}", "--acoustic-scale=1.0", "offline", str(mdl), str(wav), str(out_dir)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    tolerated = has_iv and fbank
    if p.returncode != 0 and not tolerated:
        raise RuntimeError(f"rs-dump offline failed ({p.returncode}): {p.stderr[-400:]!r}")
    d = {k: np.load(out_dir / f"{k}.npy") for k in ("loglikes", "input") + (("ivector", "chunk_tick") if has_iv else ())}
    T = d["input"].shape[0]
    fsf = int(rc.CASES[name].get("conf_opts", {}).get("frame-subsampling-factor", 1))
    assert T == rc.num_frames(name, n_samples) and d["input"].shape[1] == rc.feat_dim(name), (T, d["input"].shape, n_samples)
    assert d["loglikes"].shape[0] == (T + fsf - 1) // fsf and np.isfinite(d["loglikes"]).all() and np.isfinite(d["input"]).all()
    if has_iv:
        assert d["ivector"].shape[0] == d["chunk_tick"].shape[1] >= 1 and np.isfinite(d["ivector"]).all()
    if tolerated and p.returncode != 0:
        assert not (out_dir / "lda_norm.npy").exists()      # (it did end in the rebuild, after the four files)
    return d


def gen_case(name: str) -> None:
    case = rc.CASES[name]
    env = dict(os.environ, PATH=f"{BIN}:{os.environ['PATH']}")
    has_iv = case["spec"].get("ivector_dim", 1) > 0
    fbank = case["spec"].get("feature_type", "mfcc") == "fbank"
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        model_dir, graph_dir, wav, pcm = rc.build_case_files(name, root)
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
                cmd = ["online2-cli-nnet3-decode-faster", f"--samp-freq={rc.rate(name)}", f"--config={conf}", *decoder_args(case), str(mdl),
                       str(graph_dir / "HCLG.fst"), str(graph_dir / "words.txt"), f"ark:{lat}"]
                p = subprocess.run(cmd, env=env, input=pcm.astype("<i2").tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            out[f"{mode}_status"] = np.int32(p.returncode)
            if p.returncode != 0:
                out[f"{mode}_stderr"] = np.frombuffer(p.stderr[-400:], dtype=np.uint8)
                continue
            sh = (f"lattice-to-nbest --n={rc.NBEST} --acoustic-scale=1.0 ark:{lat} ark:- | "
                  f"nbest-to-linear ark:- ark:/dev/null ark,t:- ark,t:{root}/lm.txt ark,t:{root}/ac.txt")
            q = run(["bash", "-c", sh], env=env)
            out[f"{mode}_nbest_text"] = np.frombuffer(q.stdout, dtype=np.uint8)
            lm = parse_vec_ark((root / "lm.txt").read_text())
            ac = parse_vec_ark((root / "ac.txt").read_text())
            keys = sorted(lm, key=lambda k: int(k.split("-")[1]))
            out[f"{mode}_graph_cost"] = np.array([lm[k][0] for k in keys], np.float32)
            out[f"{mode}_acoustic_cost"] = np.array([ac[k][0] for k in keys], np.float32)
            if mode == "offline":
                d = dump_offline(name, conf, mdl, wav, root / "dump_offline", env, len(pcm), has_iv, fbank)
                out["offline_num_frames"] = np.int32(d["loglikes"].shape[0])
                out["offline_loglikes"] = d["loglikes"]
                out["input"] = d["input"]
                if has_iv:
                    out["offline_ivector"] = d["ivector"][:1]
            else:
                # the decoder's frames of the stream: one transition-id per frame on the best path of its lattice
                ali = run(["bash", "-c", f"lattice-to-nbest --n=1 --acoustic-scale=1.0 ark:{lat} ark:- | nbest-to-linear ark:- ark,t:- ark:/dev/null"], env=env)
                out["stream_num_frames"] = np.int32(len(ali.stdout.split()) - 1)
        if int(out["offline_status"]) == 0:
            assert int(out["stream_status"]) == 0 and int(out["stream_num_frames"]) == int(out["offline_num_frames"]), name
        rp = run(["rs-dump", f"--config={conf}", "randpos", str(mdl), "-", "-"], env=env)
        out["rand_calls"] = np.int64(int(rp.stdout))
        out["case_json"] = np.frombuffer(json.dumps(case, sort_keys=True).encode(), dtype=np.uint8)
        rc.GOLDEN.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(rc.GOLDEN / f"{name}.npz", **out)
        txt = bytes(out.get("offline_nbest_text", np.zeros(0, np.uint8))).decode().strip().replace("\n", " | ")
        stxt = bytes(out.get("stream_nbest_text", np.zeros(0, np.uint8))).decode().strip().replace("\n", " | ")
        rng = f" |input| <= {np.abs(out['input']).max():.4g} |loglike| <= {np.abs(out['offline_loglikes']).max():.4g}" if "input" in out else ""
        print(f"{name}: status {int(out['offline_status'])}/{int(out['stream_status'])} T={int(out.get('offline_num_frames', -1))}{rng}\n  offline: {txt}\n  stream:  {stxt}")


if __name__ == "__main__":
    for n in sys.argv[1:] or list(rc.CASES):
        gen_case(n)
