#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden alignments (runs in the build container only).

The REFERENCE's binaries (oracle/_ref, the tools oracle/build_ref.sh links) with the argv of gen_golden.py, but with
nbest-to-linear's second output -- the alignment, which the reference's pipeline sends to ark:/dev/null -- kept:
    <decoder> ... ark:LAT
    lattice-to-nbest --n=5 --acoustic-scale=1.0 ark:LAT ark:NB
    nbest-to-linear ark:NB ark,t:ALIGNMENTS ark,t:WORDS
    lattice-to-phone-lattice final.mdl ark:NB ark:- | nbest-to-linear ark:- ark:/dev/null ark,t:PHONES
for
  * every case of tests/cases.py, offline and streamed                                   case__<name>__<mode>
  * a subset of tests/search_shape_cases.py -- one graph per search the planner can choose (the 4- and 32-slot register shapes,
    exact token order, beyond the register limit) and the deepest epsilon closure -- on its two longer clips
                                                                                         shape__<name>__c<clip>__<mode>
  * the 1-, 2- and 3-frame clips of tests/length_cases.py variant V1                     len__V1__n<samples>__<mode>
  * the tiny endpoint cases of tests/endpoint_cases.py on which the reference stops early: its lattice over the frames decoded
    up to the endpoint (--online=true --do-endpointing=true, as tools/gen_endpoint_golden.py runs it)   ep__<name>
into tests/golden/alignments.npz: per record <key>__ali / __phones / __words (int32, the hypotheses back to back) with
<key>__ali_off / __phones_off / __words_off (hypothesis k = [off[k], off[k + 1])).  The big cases keep hypotheses 1 and 2 only.

Ties.  Where two alignments of a word sequence have bit-identical (total, graph) cost, which one a tool keeps is a convention.
Counting them needs the state-level lattice, and the reference's decoders refuse to write one ("--determinize-lattice=false
option is not supported at the moment", online-nnet3-decoding.cc): the determinised lattice holds one alignment per word
sequence and no trace of the ones it dropped.  So no count is printed, and tests/test_gpu_alignment.py exempts no case.

It also prints the largest |sum_t -loglike[t, pdf(tid_t)] - acoustic cost| over the non-big cases (tests/test_alignment_cpu.py
asserts it with a factor of 4).

Usage: python oracle/gen_alignment_golden.py
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "oracle"))
from rhasspy_speech_amd import synth  # noqa: E402
from tests import cases, endpoint_cases as ec, length_cases as lc, search_shape_cases as ssc  # noqa: E402
import gen_golden as gg  # noqa: E402

OUT = REPO / "tests" / "golden" / "alignments.npz"
ENV = dict(os.environ, PATH=f"{gg.BIN}:{os.environ['PATH']}")
SHAPE_CASES = ("a1024", "e4097", "exact_s1000_e2100", "s5001", "depth9")
SHAPE_CLIPS = (0, 1)
LENGTH_FRAMES = (1, 2, 3)
ENDPOINT_CASES = ("ep_tiny_u0_rule2", "ep_tiny_noiv_rule3", "ep_tiny_fsf3_rule5")
BIG_HYPS = 2


def int_ark(path: Path):
    """{key: [ints]} of a text table of integer vectors, in hypothesis order."""
    out = {}
    for line in path.read_text().splitlines():
        p = line.split()
        if p:
            out[p[0]] = [int(x) for x in p[1:]]
    return [out[k] for k in sorted(out, key=lambda k: int(k.rsplit("-", 1)[1]))]


def pack(rec: dict, key: str, name: str, lists) -> None:
    rec[f"{key}__{name}"] = np.asarray([x for l in lists for x in l], np.int32)
    rec[f"{key}__{name}_off"] = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)


def linear(root: Path, lat: Path, mdl: Path, n: int = cases.NBEST):
    """-> (alignments, words, phones, graph costs, acoustic costs) per hypothesis of the lattice table `lat`."""
    nb = root / "nb.ark"
    gg.run(["lattice-to-nbest", f"--n={n}", "--acoustic-scale=1.0", f"ark:{lat}", f"ark:{nb}"], env=ENV)
    gg.run(["nbest-to-linear", f"ark:{nb}", f"ark,t:{root}/ali.txt", f"ark,t:{root}/words.txt", f"ark,t:{root}/lm.txt", f"ark,t:{root}/ac.txt"], env=ENV)
    gg.run(["bash", "-c", f"lattice-to-phone-lattice {mdl} ark:{nb} ark:- | nbest-to-linear ark:- ark:/dev/null ark,t:{root}/phones.txt"], env=ENV)
    lm, ac = gg.parse_vec_ark((root / "lm.txt").read_text()), gg.parse_vec_ark((root / "ac.txt").read_text())
    keys = sorted(lm, key=lambda k: int(k.rsplit("-", 1)[1]))
    return (int_ark(root / "ali.txt"), int_ark(root / "words.txt"), int_ark(root / "phones.txt"), [lm[k][0] for k in keys], [ac[k][0] for k in keys])


def decode(root: Path, model_dir: Path, graph_dir: Path, wav: Path, pcm, mode: str, args):
    """The reference's decoder -> the lattice file, or None where it fails (clips without a frame)."""
    conf = model_dir / "model" / "online" / "conf" / "online.conf"
    mdl = model_dir / "model" / "model" / "final.mdl"
    lat = root / f"{mode}.lat"
    if mode == "offline":
        cmd = ["online2-wav-nnet3-latgen-faster", "--online=false", "--do-endpointing=false",
               f"--word-symbol-table={graph_dir / 'words.txt'}", f"--config={conf}", *args,
               str(mdl), str(graph_dir / "HCLG.fst"), "ark:echo utt utt|", f"scp:echo utt {wav}|", f"ark:{lat}"]
        p = subprocess.run(cmd, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    else:
        cmd = ["online2-cli-nnet3-decode-faster", f"--config={conf}", *args, str(mdl), str(graph_dir / "HCLG.fst"), str(graph_dir / "words.txt"), f"ark:{lat}"]
        p = subprocess.run(cmd, env=ENV, input=pcm.astype("<i2").tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return lat if p.returncode == 0 else None


def record(rec: dict, key: str, root: Path, model_dir: Path, graph_dir: Path, wav: Path, pcm, args, keep: int = cases.NBEST, modes=("offline", "stream")):
    mdl = model_dir / "model" / "model" / "final.mdl"
    out = {}
    for mode in modes:
        lat = decode(root, model_dir, graph_dir, wav, pcm, mode, args)
        assert lat is not None, (key, mode)
        ali, words, phones, lm, ac = linear(root, lat, mdl)
        for name, lists in (("ali", ali), ("words", words), ("phones", phones)):
            pack(rec, f"{key}__{mode}", name, lists[:keep])
        out[mode] = (ali, ac)
    return out


def main() -> None:
    rec = {}
    worst = 0.0
    # ---- tests/cases.py
    for name, case in cases.CASES.items():
        with tempfile.TemporaryDirectory() as td:
            root = Path(td)
            model_dir, graph_dir, wav, pcm = cases.build_case_files(case, root)
            got = record(rec, f"case__{name}", root, model_dir, graph_dir, wav, pcm, gg.decoder_args(case), keep=BIG_HYPS if case.get("big") else cases.NBEST)
            if not case.get("big"):
                id2pdf = synth.tid_to_pdf(cases.case_spec(case))
                with np.load(cases.GOLDEN / f"{name}.npz") as z:
                    for mode in ("offline", "stream"):
                        ll = z[f"{mode}_loglikes"].astype(np.float64)
                        for k, a in enumerate(got[mode][0]):
                            assert len(a) == ll.shape[0], (name, mode, len(a), ll.shape)
                            dev = abs(-ll[np.arange(len(a)), id2pdf[a]].sum() - float(z[f"{mode}_acoustic_cost"][k]))
                            worst = max(worst, dev)
            print(name, "frames", len(got["offline"][0][0]), "hyps", len(got["offline"][0]), flush=True)
    # ---- search shapes
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        synth.write_model_dir(root / "model", ssc.spec())
        clips = ssc.clips()
        for name in SHAPE_CASES:
            ssc.write_graph(name, root / name)
            for c in SHAPE_CLIPS:
                wav = root / "utt.wav"
                synth.write_wav(wav, clips[c])
                got = record(rec, f"shape__{name}__c{c}", root, root / "model", root / name, wav, clips[c], gg.decoder_args({"opts": {}}))
                print("shape", name, c, "frames", len(got["offline"][0][0]), "hyps", len(got["offline"][0]), flush=True)
    # ---- length edges
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        model_dir, graph_dir, pcm = lc.build_variant_files("V1", root)
        for T in LENGTH_FRAMES:
            n = lc.samples("V1", T)
            wav = root / f"n{n}.wav"
            synth.write_wav(wav, pcm[:n])
            got = record(rec, f"len__V1__n{n}", root, model_dir, graph_dir, wav, pcm[:n], gg.decoder_args(lc.case("V1")))
            assert len(got["offline"][0][0]) == T
            print("length", n, "frames", T, "hyps", len(got["offline"][0]), flush=True)
    # ---- endpoints: the lattice over the frames decoded when the reference detects the endpoint
    for name in ENDPOINT_CASES:
        g = ec.load_golden(name)
        assert g["stopped_early"], name
        with tempfile.TemporaryDirectory() as td:
            root = Path(td)
            model_dir, graph_dir, wav, pcm = ec.build_files(name, root)
            conf = model_dir / "model" / "online" / "conf" / "online.conf"
            mdl = model_dir / "model" / "model" / "final.mdl"
            lat = root / "endpoint.lat"
            base = cases.CASES[ec.ENDPOINT_CASES[name]["base"]]
            gg.run(["online2-wav-nnet3-latgen-faster", "--online=true", "--do-endpointing=true", "--chunk-length=0.064",
                    f"--word-symbol-table={graph_dir / 'words.txt'}", f"--config={conf}", *gg.decoder_args(base),
                    str(mdl), str(graph_dir / "HCLG.fst"), "ark:echo utt utt|", f"scp:echo utt {wav}|", f"ark:{lat}"], env=ENV)
            ali, words, phones, _, _ = linear(root, lat, mdl)
            assert len(ali[0]) == g["frames"] and words == [h["words"] for h in g["nbest"]], name
            for nm, lists in (("ali", ali), ("words", words), ("phones", phones)):
                pack(rec, f"ep__{name}", nm, lists)
            print("endpoint", name, "frames", len(ali[0]), "hyps", len(ali), flush=True)
    np.savez_compressed(OUT, **rec)
    print(f"{OUT.name}: {OUT.stat().st_size} bytes, {len(rec)} arrays")
    print(f"largest |sum of -loglike over the alignment - acoustic cost| on the non-big cases: {worst:.3e}")


if __name__ == "__main__":
    main()
