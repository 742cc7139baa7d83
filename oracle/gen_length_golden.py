#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- goldens of the utterance-length edge cases (tests/length_cases.py; runs in the build container only).

Every case runs the reference's binaries exactly as oracle/gen_golden.py does (run_reference: online2-wav-nnet3-latgen-faster |
lattice-to-nbest --n=5 | nbest-to-linear offline, online2-cli-nnet3-decode-faster streamed, rs-dump for features, iVectors, chunk
ticks and log-likelihoods) on a prefix of the variant's utterance.  One tests/golden/lengths/<variant>.npz per variant (where that
would be larger than a committed file may be, the streamed runs' arrays go to <variant>_stream.npz beside it); the arrays
of the case of n samples are named n<n>_<what run_reference calls them>.  Log-likelihoods are kept in full up to 49 frames; longer
cases (the CMVN edges) keep every 8th row and the last 8, with the kept row indices beside them (n<n>_<mode>_loglike_rows).
Features that are the first rows of the longest clip's are stored once (see gen_variant).

Usage: python oracle/gen_length_golden.py [variant ...]
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle.gen_golden import BIN, run_reference  # noqa: E402
from rhasspy_speech_amd import synth  # noqa: E402
from tests import length_cases as lc  # noqa: E402

FULL_ROWS_UP_TO = 49
MAX_BYTES = 1 << 20          # no committed file of this repository may be larger


def kept_rows(T: int) -> np.ndarray:
    return np.array(sorted(set(range(0, T, 8)) | set(range(T - 8, T))), np.int32)


def gen_length(case: dict, model_dir: Path, graph_dir: Path, pcm: np.ndarray, n: int, env: dict) -> dict:
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        clip = pcm[:n]
        wav = root / "utt.wav"
        synth.write_wav(wav, clip)
        out = run_reference(case, root, model_dir, graph_dir, wav, clip, env)
    for k in ("cmvn", "lda", "lda_norm"):      # (the iVector branch's intermediates: pinned on tests/golden/tiny_u0.npz)
        out.pop(k, None)
    for mode in ("offline", "stream"):
        ll = out.get(f"{mode}_loglikes")
        if ll is not None and ll.shape[0] > FULL_ROWS_UP_TO:
            rows = kept_rows(ll.shape[0])
            out[f"{mode}_loglikes"] = ll[rows].copy()
            out[f"{mode}_loglike_rows"] = rows
    return {f"{lc.key(n)}_{k}": v for k, v in out.items()}


def gen_variant(variant: str) -> None:
    env = dict(os.environ, PATH=f"{BIN}:{os.environ['PATH']}")
    case = lc.case(variant)
    with tempfile.TemporaryDirectory() as td:
        model_dir, graph_dir, pcm = lc.build_variant_files(variant, Path(td))
        ns = list(lc.lengths(variant))
        with ThreadPoolExecutor(max_workers=int(os.environ.get("JOBS", "8"))) as pool:
            parts = list(pool.map(lambda n: gen_length(case, model_dir, graph_dir, pcm, n, env), ns))
    out = {}
    for p in parts:
        out.update(p)
    # the clips are prefixes of one utterance and the dither of frame t is seeded by t: where the features of a clip are, bit for
    # bit, the first rows of the longest clip's, only that is stored (n<n>_input_of = the longer clip; tests.length_cases.load_golden
    # puts the rows back)
    have = [n for n in ns if f"{lc.key(n)}_input" in out]
    if have:
        longest = out[f"{lc.key(have[-1])}_input"]
        for n in have[:-1]:
            a = out[f"{lc.key(n)}_input"]
            if np.array_equal(a.view(np.uint32), longest[:a.shape[0]].view(np.uint32)):
                del out[f"{lc.key(n)}_input"]
                out[f"{lc.key(n)}_input_of"] = np.array([have[-1], a.shape[0]], np.int32)      # (clip, rows)
    out["lengths"] = np.array(ns, np.int32)
    out["case_json"] = np.frombuffer(json.dumps(case, sort_keys=True).encode(), dtype=np.uint8)
    lc.GOLDEN.mkdir(parents=True, exist_ok=True)
    path = lc.GOLDEN / f"{variant}.npz"
    np.savez_compressed(path, **out)
    size = path.stat().st_size
    second = lc.GOLDEN / f"{variant}_stream.npz"
    second.unlink(missing_ok=True)
    if size > MAX_BYTES:      # (the zamia-size variant: 2000 pdfs a row) the streamed runs' arrays in a file of their own
        np.savez_compressed(path, **{k: v for k, v in out.items() if "_stream_" not in k})
        np.savez_compressed(second, **{k: v for k, v in out.items() if "_stream_" in k})
        size = max(path.stat().st_size, second.stat().st_size)
    failed = [n for n in ns if int(out[f"{lc.key(n)}_offline_status"]) != 0]
    print(f"{variant}: {len(ns)} lengths, {size} bytes, no lattice offline at n = {failed}")
    for n in ns:
        st = [int(out[f"{lc.key(n)}_{m}_status"]) for m in ("offline", "stream")]
        txt = bytes(out.get(f"{lc.key(n)}_offline_nbest_text", np.zeros(0, np.uint8))).decode().strip().replace("\n", " | ")
        print(f"  n={n} {lc.lengths(variant)[n]} status={st} T={int(out.get(f'{lc.key(n)}_offline_num_frames', 0))}: {txt[:100]}")
    assert size <= MAX_BYTES, (variant, size)


if __name__ == "__main__":
    for v in sys.argv[1:] or list(lc.VARIANTS):
        gen_variant(v)
