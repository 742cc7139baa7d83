"""The search-shape graph family (tests/search_shape_cases.py) without a GPU.

1. Every case lands on the kernel shape, lattice rung, closure mode and lattice route its row of the table names -- by the real
   planner: tests/host/search_plan_check.cc, built under the address and undefined-behaviour sanitizers, reads the graph's arcs
   (`--graph`) and prints WalkSearchGraph, DescribeSearchLoad (the `search:` line of rs_model_describe) and DescribeSearchCall.
2. The Python walker of the case module agrees with WalkSearchGraph on every graph.
3. The CPU oracle (oracle/decoder.c behind pipeline.Oracle) gives the reference binaries' 5-best lists and costs on every case,
   option set and clip (tests/golden/search_shapes.json, oracle/gen_search_shape_golden.py): word sequences exact, costs
   rtol=2e-4 / atol=2e-3, the suite's tolerance against the reference.  The graphs go to epsilon depth 9.
4. The depth cases are sensitive to the closure: the 1-best graph cost is that of the graph without shortcuts (the chain is always
   the way taken), and differs by at least 0.9 from that of the graph whose chains are cut (the shortcut costs 1.0 per word more).
5. The reference's lists on the family's inputs do not depend on the order in which its decoder creates tokens (the kernels prune
   with the final cutoff); the one combination found that does is pinned."""
import json
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rhasspy_speech_amd import synth

from . import cases
from . import search_shape_cases as ssc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
GOLD = json.loads((cases.GOLDEN / "search_shapes.json").read_text())
CUS = 256
# (n_utts, nbest, exact_token_order) of the calls planned per case: a batch of three, its n-best call, the exact order, and both
# sides of the crowded threshold (4 n_utts >= 3 CUs: 192 of 256)
CALLS = ((3, 1, 0), (3, 5, 0), (3, 1, 1), (191, 1, 0), (192, 1, 0), (191, 1, 1), (192, 1, 1))
CROWDED = {"<512,4,2>": "<256,8,4>", "<512,8,4>": "<256,16,8>"}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """case -> (the walk line's fields, the search: line, {call: DescribeSearchCall}); under RS_LATTICE_KERNEL=vote: "vote" -> {call: ...}"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("search_shapes")
    exe = tmp / "search_plan_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "search_plan_check.cc"), str(CSRC / "search_plan.cc"), "-o", str(exe)], check=True)
    out = {}
    env = {k: v for k, v in os.environ.items() if not k.startswith("RS_")}
    for name in ssc.CASES:
        arcs = tmp / f"{name}.arcs"
        ssc.write_arcs_file(arcs, ssc.build(name)[0], ssc.spec().num_pdfs)
        args = [str(exe), "--graph", str(arcs), str(CUS)] + [str(v) for c in CALLS for v in c]
        p = subprocess.run(args, capture_output=True, text=True, env=env)
        assert p.returncode == 0 and p.stderr == "", (name, p.returncode, p.stderr[-4000:])
        lines = p.stdout.splitlines()
        assert len(lines) == 2 + len(CALLS) and lines[0].startswith("walk: ") and lines[1].startswith("search: ")
        walk = {k: int(v) for k, v in (f.split("=") for f in lines[0].split()[1:])}
        calls = {c: l.split(" | ", 1)[1] for c, l in zip(CALLS, lines[2:])}
        p = subprocess.run(args[:4] + ["3", "5", "0"], capture_output=True, text=True, env=dict(env, RS_LATTICE_KERNEL="vote"))
        assert p.returncode == 0 and p.stderr == "", (name, p.stderr[-4000:])
        out[name] = (walk, lines[1], calls, p.stdout.splitlines()[2].split(" | ", 1)[1])
    return out


@pytest.mark.parametrize("name", list(ssc.CASES))
def test_case_lands_where_its_row_says(plans, name):
    c = ssc.CASES[name]
    walk, line, calls, vote = plans[name]
    # the line rs_model_describe reports, field by field what the table says
    assert line == ssc.search_line(name, crowded_at=192)
    assert f" reg={c['reg']} eps_rounds={c['rounds']} exact_ok={c['exact_ok']} dense_ok=1 dense_lattice={c['dl']} crowded_at=192" in line
    best, nbest, exact = calls[(3, 1, 0)], calls[(3, 5, 0)], calls[(3, 1, 1)]
    if c["reg"] == "none":      # one state beyond the register-resident search: the LDS-resident dense one, token lists for a lattice
        assert best.startswith("dense DenseDecode<256,") and exact.startswith("dense ")
        assert nbest.startswith("live LiveDecode<1024>") and " | lattice=tokens | " in nbest
        assert calls[(192, 1, 0)].startswith("dense ")
        return
    assert best.startswith(f"reg RegDecode{c['reg']} grid=3 threads={c['reg'][1:4]} ")
    assert nbest.startswith(f"reg RegDecode{c['reg']} ")
    if c["route"] == "dense-rows":
        assert f" | lattice=dense-rows DenseLattice{c['dl']} grid=3 threads=512 " in nbest and f" eps_rounds={c['rounds']} | " in nbest
        # RS_LATTICE_KERNEL=vote: the lattice kernel's closure runs until nothing changes, unless the graph has no epsilon arc
        assert f" eps_rounds={-1 if c['rounds'] != 0 else 0} | " in vote and f"DenseLattice{c['dl']} " in vote
    else:
        assert c["dl"] == "none" and f" | lattice={c['route']} | " in nbest and f" | lattice={c['route']} | " in vote
    # the exact token order, where the graph allows it
    kernel = "RegDecodeExact" if c["exact_ok"] else "RegDecode"
    assert exact.startswith(f"{'reg-exact' if c['exact_ok'] else 'reg'} {kernel}{c['reg']} "), exact
    # the crowded rule at 256 CUs: 191 utterances keep the shape, 192 get half the waves and twice the arcs per thread
    crowded = CROWDED.get(c["reg"], c["reg"])
    assert calls[(191, 1, 0)].startswith(f"reg RegDecode{c['reg']} grid=191 ")
    assert calls[(192, 1, 0)].startswith(f"reg RegDecode{crowded} grid=192 threads=256 ")
    assert calls[(191, 1, 1)].startswith(f"{'reg-exact' if c['exact_ok'] else 'reg'} {kernel}{c['reg']} grid=191 ")
    assert calls[(192, 1, 1)].startswith(f"{'reg-exact' if c['exact_ok'] else 'reg'} {kernel}{crowded} grid=192 ")


def test_the_table_covers_every_shape_rung_and_closure_mode():
    """What the family is for: together with the 625-state graph of the other tests (<512,4,2>, rung 4 or 6, one round)."""
    regs = {c["reg"] for c in ssc.CASES.values()}
    assert regs == {"<512,4,2>", "<512,8,4>", "<256,32,16>", "none"}      # <256,8,4> and <256,16,8>: the crowded batches of CROWDED_CASES
    assert {ssc.CASES[n]["reg"] for n in ssc.CROWDED_CASES} == set(CROWDED)
    assert {c["dl"] for c in ssc.CASES.values()} == {f"<512,{k}>" for k in (2, 4, 6, 8, 12, 16)} | {"none"}
    for route in ("dense-rows", "rows-to-tokens"):
        assert {c["rounds"] for c in ssc.CASES.values() if c["route"] == route} >= {1, 3, -1}
    assert {c["rounds"] for c in ssc.CASES.values() if c["route"] == "dense-rows"} == {0, 1, 2, 3, 6, -1}
    assert {ssc.CASES[n]["reg"] for n in ssc.CASES if ssc.CASES[n]["exact_ok"]} == {"<512,4,2>", "<512,8,4>"}
    assert set(ssc.STREAM_CASES) | set(ssc.CROWDED_CASES) | set(ssc.DEPTH_CASES) <= set(ssc.CASES)


@pytest.mark.parametrize("name", list(ssc.CASES))
def test_python_walker_agrees_with_the_planner(plans, name):
    w = plans[name][0]
    assert ssc.walk(ssc.build(name)[0]) == (w["states"], w["in_e"], w["in_x"], w["eps_depth"], w["max_out_e"], w["max_out_x"])


def test_limits_are_met_exactly():
    want = {"e2048_x1024": (None, 2048, 1024), "e2049": (None, 2049, 1024), "x1025": (None, 2048, 1025), "e4096_x2048": (None, 4096, 2048),
            "e4097": (None, 4097, None), "a8192_s2048": (2048, None, None), "s2049": (2049, None, None), "e8192_x4096": (None, 8192, 4096),
            "s5000": (5000, None, None), "s5001": (5001, None, None), "exact_s1000_e2100": (1000, 2100, None), "exact_s1001": (1001, None, None)}
    for name, (S, e, x) in want.items():
        got = ssc.walk(ssc.build(name)[0])
        assert (S is None or got[0] == S) and (e is None or got[1] == e) and (x is None or got[2] == x), (name, got)
    for name, arcs in (("a8192_s2048", 8192), ("s2049", 8192), ("a1024", 1024), ("a1025", 1025), ("e2048_x1024", 3072), ("e4096_x2048", 6144)):
        got = ssc.walk(ssc.build(name)[0])
        assert got[1] + got[2] == arcs, (name, got)
    assert ssc.walk(ssc.build("out32")[0])[4:] == (32, 32)
    for name in ssc.CASES:
        S = ssc.walk(ssc.build(name)[0])[0]
        assert S <= ssc.CASES[name].get("S_max", S)
    for name in ("e2048_x1024", "e2049", "x1025", "out32", "exact_s1000_e2100"):
        assert ssc.walk(ssc.build(name)[0])[0] <= 1000
    assert ssc.walk(ssc.build("depth0")[0])[2] == 0


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("search_shape_files")
    synth.write_model_dir(root / "model", ssc.spec())
    built = {}

    def graph(name, variant="full"):
        if (name, variant) not in built:
            built[name, variant] = root / f"{name}_{variant}"
            ssc.write_graph(name, built[name, variant], variant)
        return root / "model", built[name, variant]

    return graph


@pytest.mark.parametrize("oname", list(ssc.OPTION_SETS))
@pytest.mark.parametrize("name", list(ssc.CASES))
def test_oracle_is_the_reference(dirs, name, oname):
    from oracle import pipeline
    model_dir, graph_dir = dirs(name)
    orc = pipeline.Oracle(model_dir, graph_dir, **ssc.OPTION_SETS[oname])
    for u, pcm in enumerate(ssc.clips()):
        for mode, run in (("offline", orc.transcribe), ("stream", orc.transcribe_stream)):
            gold = GOLD[name][oname][u][mode]
            assert gold["status"] == 0
            tr = run(pcm, nbest=ssc.NBEST)
            ref = [[int(w) for w in l.split()[1:]] for l in gold["nbest_text"].splitlines() if l.split()]
            assert [p.words for p in tr.nbest] == ref, (name, oname, u, mode)
            if u < 2:
                assert ref[0], (name, oname, u, mode)
            np.testing.assert_allclose([p.graph_cost for p in tr.nbest], gold["graph_cost"], rtol=2e-4, atol=2e-3)
            np.testing.assert_allclose([p.acoustic_cost for p in tr.nbest], gold["acoustic_cost"], rtol=2e-4, atol=2e-3)


def _lists(tr):
    return [p.words for p in tr.nbest], [p.graph_cost for p in tr.nbest], [p.acoustic_cost for p in tr.nbest]


@pytest.mark.parametrize("name", list(ssc.CASES))
def test_reference_lists_do_not_hang_on_token_order(dirs, name, monkeypatch):
    """The kernels prune with each frame's final cutoff, the reference while its running cutoff tightens, so which tokens beyond
    the cutoff exist follows its hash order ("order-dependent extras").  oracle/decoder.c does either
    (RS_ORACLE_FINAL_CUTOFF=1: the kernels' rule); on the family's inputs both give the same 5-best lists, so the reference's are
    the kernels' target to the suite's tolerance.  (The exact token order closes the gap only up to closure depth 1.)"""
    from oracle import pipeline
    model_dir, graph_dir = dirs(name)
    for oname, opts in ssc.OPTION_SETS.items():
        orc = pipeline.Oracle(model_dir, graph_dir, **opts)
        for u, pcm in enumerate(ssc.clips()):
            for run in (orc.transcribe, orc.transcribe_stream)[:2 if u == 0 else 1]:
                monkeypatch.setenv("RS_ORACLE_FINAL_CUTOFF", "0")
                a = _lists(run(pcm, nbest=ssc.NBEST))
                monkeypatch.setenv("RS_ORACLE_FINAL_CUTOFF", "1")
                b = _lists(run(pcm, nbest=ssc.NBEST))
                assert a[0] == b[0], (name, oname, u)
                np.testing.assert_allclose(a[1], b[1], rtol=2e-6, atol=1e-4)
                np.testing.assert_allclose(a[2], b[2], rtol=2e-6, atol=1e-4)


def test_the_pinned_order_dependent_list(dirs, monkeypatch):
    """ssc.ORDER_DEPENDENT: the oracle in the reference's order gives the reference's five hypotheses, with the final cutoff the
    first three of them and one token less."""
    from oracle import pipeline
    od = ssc.ORDER_DEPENDENT
    gold = GOLD["order_dependent"]["offline"]
    model_dir, graph_dir = dirs(od["case"])
    orc = pipeline.Oracle(model_dir, graph_dir, **ssc.OPTION_SETS[od["options"]])
    pcm = synth.synth_utterance(*od["clip"])
    monkeypatch.setenv("RS_ORACLE_FINAL_CUTOFF", "0")
    ref = orc.transcribe(pcm, nbest=ssc.NBEST)
    monkeypatch.setenv("RS_ORACLE_FINAL_CUTOFF", "1")
    fin = orc.transcribe(pcm, nbest=ssc.NBEST)
    want = [[int(w) for w in l.split()[1:]] for l in gold["nbest_text"].splitlines() if l.split()]
    assert (len(want), len(fin.nbest)) == od["hyps"]
    assert _lists(ref)[0] == want and _lists(fin)[0] == want[:len(fin.nbest)]
    np.testing.assert_allclose(_lists(ref)[1], gold["graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(_lists(fin)[1], gold["graph_cost"][:len(fin.nbest)], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(_lists(fin)[2], gold["acoustic_cost"][:len(fin.nbest)], rtol=2e-4, atol=2e-3)
    assert fin.counters[2] == ref.counters[2] - 1


@pytest.mark.parametrize("name", ssc.DEPTH_CASES)
def test_depth_cases_are_sensitive_to_the_closure(dirs, name):
    from oracle import pipeline
    pcm = ssc.clips()[0]
    best = {}
    for variant in ("full", "no_shortcut", "broken"):
        model_dir, graph_dir = dirs(name, variant)
        best[variant] = pipeline.Oracle(model_dir, graph_dir).transcribe(pcm).nbest[0]
    assert best["full"].words and best["full"].words == best["no_shortcut"].words
    assert best["full"].graph_cost == best["no_shortcut"].graph_cost
    print(name, {v: (p.words, p.graph_cost, p.acoustic_cost) for v, p in best.items()})
    assert abs(best["broken"].graph_cost - best["full"].graph_cost) >= 0.9
