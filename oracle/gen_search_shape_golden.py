#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for the search-shape graph family (build container only).

tests/search_shape_cases.py builds one graph per kernel shape, closure depth and limit of the search planner.  For every case,
option set and clip the REFERENCE's binaries (oracle/_ref) are run exactly as gen_fuzz_decode_golden.py runs them --
`online2-wav-nnet3-latgen-faster | lattice-to-nbest --n=5 | nbest-to-linear` and the streaming `online2-cli-nnet3-decode-faster`
-- and their exit status, 5-best text, graph costs and acoustic costs are stored in tests/golden/search_shapes.json:
    {case: {option set: [per clip {"offline": {...}, "stream": {...}}]}}
Every status must be 0 and the two longer clips of every case must have a 1-best with words in it: the script fails otherwise.

Usage: python oracle/gen_search_shape_golden.py [case ...]      (named cases replace their records in the existing file)
"""
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "oracle"))
from rhasspy_speech_amd import synth  # noqa: E402
from tests import search_shape_cases as ssc  # noqa: E402
import gen_golden as gg  # noqa: E402

OUT = REPO / "tests" / "golden" / "search_shapes.json"
ENV = dict(os.environ, PATH=f"{gg.BIN}:{os.environ['PATH']}")


def run_clip(root: Path, model_dir: Path, graph_dir: Path, opts: dict, pcm) -> dict:
    conf = model_dir / "model" / "online" / "conf" / "online.conf"
    mdl = model_dir / "model" / "model" / "final.mdl"
    wav = root / "utt.wav"
    synth.write_wav(wav, pcm)
    args = gg.decoder_args({"opts": opts})
    out = {}
    for mode in ("offline", "stream"):
        lat = root / f"{mode}.lat"
        if mode == "offline":
            cmd = ["online2-wav-nnet3-latgen-faster", "--online=false", "--do-endpointing=false",
                   f"--word-symbol-table={graph_dir / 'words.txt'}", f"--config={conf}", *args,
                   str(mdl), str(graph_dir / "HCLG.fst"), "ark:echo utt utt|", f"scp:echo utt {wav}|", f"ark:{lat}"]
            p = subprocess.run(cmd, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        else:
            cmd = ["online2-cli-nnet3-decode-faster", f"--config={conf}", *args, str(mdl),
                   str(graph_dir / "HCLG.fst"), str(graph_dir / "words.txt"), f"ark:{lat}"]
            p = subprocess.run(cmd, env=ENV, input=pcm.astype("<i2").tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if p.returncode != 0:
            out[mode] = {"status": p.returncode}
            continue
        sh = (f"lattice-to-nbest --n={ssc.NBEST} --acoustic-scale=1.0 ark:{lat} ark:- | "
              f"nbest-to-linear ark:- ark:/dev/null ark,t:- ark,t:{root}/lm.txt ark,t:{root}/ac.txt")
        q = gg.run(["bash", "-c", sh], env=ENV)
        lm = gg.parse_vec_ark((root / "lm.txt").read_text())
        ac = gg.parse_vec_ark((root / "ac.txt").read_text())
        keys = sorted(lm, key=lambda k: int(k.split("-")[1]))
        out[mode] = {"status": 0, "nbest_text": q.stdout.decode(), "graph_cost": [lm[k][0] for k in keys], "acoustic_cost": [ac[k][0] for k in keys]}
    return out


def main():
    names = sys.argv[1:] or list(ssc.CASES)
    recs = json.loads(OUT.read_text()) if sys.argv[1:] and OUT.exists() else {}
    bad = []
    with tempfile.TemporaryDirectory() as td:
        root = Path(td)
        synth.write_model_dir(root / "model", ssc.spec())
        for name in names:
            ssc.write_graph(name, root / name)
            recs[name] = {}
            for oname, opts in ssc.OPTION_SETS.items():
                recs[name][oname] = [run_clip(root, root / "model", root / name, opts, pcm) for pcm in ssc.clips()]
                for u, r in enumerate(recs[name][oname]):
                    for mode in ("offline", "stream"):
                        first = r[mode].get("nbest_text", "").splitlines()[:1]
                        if r[mode]["status"] != 0 or (u < 2 and not (first and first[0].split()[1:])):
                            bad.append((name, oname, u, mode, r[mode]["status"]))
                print(name, oname, "->", " / ".join(r["offline"].get("nbest_text", "status").split("\n")[0] for r in recs[name][oname]), flush=True)
        # the pinned order-dependent combination (ssc.ORDER_DEPENDENT): the reference's list, offline
        od = ssc.ORDER_DEPENDENT
        ssc.write_graph(od["case"], root / od["case"])
        recs["order_dependent"] = run_clip(root, root / "model", root / od["case"], ssc.OPTION_SETS[od["options"]], synth.synth_utterance(*od["clip"]))
        assert recs["order_dependent"]["offline"]["status"] == 0
    OUT.write_text(json.dumps({n: recs[n] for n in list(ssc.CASES) + ["order_dependent"] if n in recs}, indent=0))
    assert not bad, bad


if __name__ == "__main__":
    main()
