"""Every kernel shape, closure depth and limit the search planner can choose, launched on the GPU and checked.

tests/search_shape_cases.py builds one graph per row (tests/test_search_shapes_cpu.py holds each to the real planner and the CPU
oracle to the reference's binaries on all of them).  Here, for every case and two option sets (the defaults, and pruning options
that bind on most frames):
  1. the `search:` line of rs_model_describe is the one the case table implies -- a case that drifts onto another kernel fails;
  2. the 5-best lists of a batch call are the reference binaries' (tests/golden/search_shapes.json): text exact, costs
     rtol=2e-4 / atol=2e-3, as every test against the reference;
  3. the 1-best is the sequential decoder's (oracle/decoder.c) on the device's own log-likelihoods; with exact_token_order, where
     the graph allows it, costs and work counters as test_exact_token_order_is_the_sequential_decoder compares them;
  4. the token-list search (RS_DECODER=sparse), which has no shapes, against the automatic choice, the LDS-resident dense search and
     the live-state table: words, costs rtol=1e-6, counters -- all four run their epsilon closure on the deep graphs;
  5. the lattice routes (DenseLatticeKernel counted / voting, rows to tokens, token-list search) leave the same lattice;
  6. streams (five cases): the finish is the reference's streamed result, a partial the oracle's best path so far;
  7. crowded batches (4 n_utts >= 3 CUs) run RegDecode<256,8,4> / <256,16,8> and RegDecodeExact<256,8,4>: every utterance bit for
     bit as in a batch of three.
An eighth test pins the one order-dependent list met while the clips were chosen (ssc.ORDER_DEPENDENT).
Measured on one MI355X: 198 tests, the whole file in 16.5 s; the slowest test 1.1 s."""
import json

import numpy as np
import pytest

from . import cases
from . import search_shape_cases as ssc

pytestmark = pytest.mark.gpu

GOLD = json.loads((cases.GOLDEN / "search_shapes.json").read_text())
PARAMS = [(n, o) for n in ssc.CASES for o in ssc.OPTION_SETS]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (model_dir, graph_dir): one acoustic model for the family, one graph directory per case."""
    from rhasspy_speech_amd import synth
    root = tmp_path_factory.mktemp("search_shapes")
    synth.write_model_dir(root / "model", ssc.spec())
    built = {}

    def get(name):
        if name not in built:
            ssc.write_graph(name, root / name)
            built[name] = (root / "model", root / name)
        return built[name]

    return get


def _crowded_at():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (3 * cus + 3) // 4


def _model(files, name, oname, **extra):
    """The case's model with the option set; its search: line must be the table's whatever the test goes on to check."""
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir = files(name)
    o = dict(keep_intermediates=1)
    o.update(ssc.OPTION_SETS[oname])
    o.update(extra)
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(**o))
    model.to_device()
    lines = [l for l in model.describe().splitlines() if l.startswith("search: ")]
    assert lines == [ssc.search_line(name, _crowded_at())], (lines, ssc.search_line(name, _crowded_at()))
    return model


def _check_golden(res, u, gold, what):
    assert gold["status"] == 0
    assert res.text(u, "utt").split() == gold["nbest_text"].encode().split(), what
    n = len(gold["graph_cost"])
    assert res.num_hyps(u) == n, what
    gc = np.array([res.costs(u, k)[0] for k in range(n)])
    ac = np.array([res.costs(u, k)[1] for k in range(n)])
    np.testing.assert_allclose(gc, gold["graph_cost"], rtol=2e-4, atol=2e-3, err_msg=what)
    np.testing.assert_allclose(ac, gold["acoustic_cost"], rtol=2e-4, atol=2e-3, err_msg=what)


@pytest.mark.parametrize("name,oname", PARAMS)
def test_nbest_is_the_reference(files, name, oname):
    model = _model(files, name, oname)
    res = model.decode_batch(ssc.clips(), nbest=ssc.NBEST)
    for u in range(len(ssc.CLIPS)):
        _check_golden(res, u, GOLD[name][oname][u]["offline"], f"{name} {oname} clip {u}")
    model.close()


def test_order_dependent_extras_are_the_final_cutoffs(files, monkeypatch):
    """ssc.ORDER_DEPENDENT (max-active binds on a 6-frame clip, closure depth 7: no exact token order): the reference lists five
    hypotheses, two of them through a token it created above the final cutoff of its frame.  The kernels give the sequential
    decoder's list under the final cutoff -- the first three -- at the reference's costs."""
    from oracle import pipeline
    from rhasspy_speech_amd import synth
    od = ssc.ORDER_DEPENDENT
    gold = GOLD["order_dependent"]["offline"]
    model_dir, graph_dir = files(od["case"])
    model = _model(files, od["case"], od["options"])
    res = model.decode_batch([synth.synth_utterance(*od["clip"])], nbest=ssc.NBEST)
    want = gold["nbest_text"].encode().split(b"\n")
    assert (len(gold["graph_cost"]), res.num_hyps(0)) == od["hyps"]
    n = res.num_hyps(0)
    assert res.text(0, "utt").split() == b" ".join(want[:n]).split()
    np.testing.assert_allclose([res.costs(0, k)[0] for k in range(n)], gold["graph_cost"][:n], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose([res.costs(0, k)[1] for k in range(n)], gold["acoustic_cost"][:n], rtol=2e-4, atol=2e-3)
    monkeypatch.setenv("RS_ORACLE_FINAL_CUTOFF", "1")
    orc = pipeline.Oracle(model_dir, graph_dir, **ssc.OPTION_SETS[od["options"]])
    lattice, _ = pipeline.decode(orc.fst, orc.id2pdf, res.matrix(0, 2), **orc.opts)
    paths = pipeline.lat.nbest(lattice, ssc.NBEST, orc.opts["lattice_beam"], 1.0)
    assert [res.words(0, k) for k in range(n)] == [p.words for p in paths]
    model.close()


@pytest.mark.parametrize("name,oname", PARAMS)
def test_best_path_is_the_sequential_decoders(files, name, oname):
    from oracle import pipeline
    model_dir, graph_dir = files(name)
    orc = pipeline.Oracle(model_dir, graph_dir, **ssc.OPTION_SETS[oname])
    pcms = ssc.clips()
    model = _model(files, name, oname)
    res = model.decode_batch(pcms)
    seq = []
    for u in range(len(pcms)):
        lattice, ctr = pipeline.decode(orc.fst, orc.id2pdf, res.matrix(u, 2), **orc.opts)
        seq.append((pipeline.lat.nbest(lattice, 1, orc.opts["lattice_beam"], 1.0)[0], ctr))
        assert res.words(u) == seq[u][0].words, u
    model.close()
    if not ssc.CASES[name]["exact_ok"]:
        return
    model = _model(files, name, oname, exact_token_order=1)
    assert "token_order: exact" in model.describe(), model.describe()
    got = model.decode_batch(pcms)
    for u, (best, ctr) in enumerate(seq):
        np.testing.assert_array_equal(got.matrix(u, 2), res.matrix(u, 2))
        assert got.words(u) == best.words
        np.testing.assert_allclose(got.costs(u), (best.graph_cost, best.acoustic_cost), rtol=2e-6, atol=1e-4)
        assert got.counters(u)[5] == ctr[5] and got.counters(u)[6] == ctr[6], (got.counters(u), ctr)
        assert got.counters(u)[3] == ctr[3] + ctr[7], (got.counters(u), ctr)
    model.close()


@pytest.mark.parametrize("name,oname", PARAMS)
def test_searches_agree_with_the_token_list_search(files, name, oname, monkeypatch):
    pcms = ssc.clips()
    res = {}
    for variant in ("sparse", "auto", "dense", "hash"):
        if variant == "auto":
            monkeypatch.delenv("RS_DECODER", raising=False)
        else:
            monkeypatch.setenv("RS_DECODER", variant)
        model = _model(files, name, oname)
        res[variant] = model.decode_batch(pcms)
        model.close()
    monkeypatch.delenv("RS_DECODER", raising=False)
    ref = res["sparse"]
    for variant in ("auto", "dense", "hash"):
        got = res[variant]
        for u in range(len(pcms)):
            assert got.words(u) == ref.words(u), (variant, u)
            np.testing.assert_allclose(got.costs(u), ref.costs(u), rtol=1e-6, err_msg=f"{variant} {u}")
            assert got.counters(u)[3] == ref.counters(u)[3], (variant, u)
            assert got.counters(u)[5] == ref.counters(u)[5] and got.counters(u)[6] == ref.counters(u)[6], (variant, u)


@pytest.mark.parametrize("name,oname", PARAMS)
def test_lattice_routes_leave_the_same_lattice(files, name, oname, monkeypatch):
    pcms = ssc.clips()
    model = _model(files, name, oname)
    routes = {"default": {}, "tokens-kernel": {"RS_LATTICE_KERNEL": "tokens"}, "tokens-search": {"RS_LATTICE_SEARCH": "tokens"}}
    if ssc.CASES[name]["dl"] != "none":
        routes["vote"] = {"RS_LATTICE_KERNEL": "vote"}
    res = {}
    for route, env in routes.items():
        for k in ("RS_LATTICE_KERNEL", "RS_LATTICE_SEARCH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res[route] = model.decode_batch(pcms, nbest=ssc.NBEST)
    for k in ("RS_LATTICE_KERNEL", "RS_LATTICE_SEARCH"):
        monkeypatch.delenv(k, raising=False)
    ref = res["tokens-search"]
    for route in routes:
        got = res[route]
        for u in range(len(pcms)):
            assert got.num_hyps(u) == ref.num_hyps(u), (route, u)
            assert got.counters(u)[4] == ref.counters(u)[4], (route, u)          # arcs of the raw lattice
            for k in range(ref.num_hyps(u)):
                assert got.words(u, k) == ref.words(u, k), (route, u, k)
                np.testing.assert_allclose(got.costs(u, k), ref.costs(u, k), rtol=1e-6, err_msg=f"{route} {u} {k}")
    model.close()


@pytest.mark.parametrize("name,oname", [(n, o) for n in ssc.STREAM_CASES for o in ssc.OPTION_SETS])
def test_stream_is_the_reference_and_its_partial_the_oracles(files, name, oname):
    from oracle import pipeline
    from rhasspy_speech_amd import _lib
    from .test_gpu_stream_partial import COST_ATOL, COST_RTOL, _oracle_best
    model_dir, graph_dir = files(name)
    model = _model(files, name, oname)
    st = _lib.Stream(model)
    raw = ssc.clips()[0].tobytes()
    part = None
    for i, k in enumerate(range(0, len(raw), 8192)):
        st.accept(raw[k:k + 8192])
        st.advance()
        if i == 1:
            r = st.partial()
            assert r.num_utts == 1 and r.num_hyps(0) == 1
            part = (r.num_frames(0), r.words(0), r.costs(0))
            r.close()
    res = st.finish(ssc.NBEST, 1.0)
    _check_golden(res, 0, GOLD[name][oname][0]["stream"], f"{name} {oname} stream")
    n, words, costs = part
    assert 0 < n <= res.num_frames(0)
    orc = pipeline.Oracle(model_dir, graph_dir, **ssc.OPTION_SETS[oname])
    best = _oracle_best(orc, res.matrix(0, 2), n)
    assert words == best.words, (n, words, best.words)
    np.testing.assert_allclose(costs, (best.graph_cost, best.acoustic_cost), rtol=COST_RTOL, atol=COST_ATOL)
    model.close()


@pytest.mark.parametrize("name,exact", [(ssc.CROWDED_CASES[0], 0), (ssc.CROWDED_CASES[1], 0), (ssc.CROWDED_CASES[0], 1)])
def test_crowded_batch_is_the_batch_of_three(files, name, exact):
    """crowded_at utterances: the planner halves the waves and doubles the arcs per thread (<512,4,2> -> <256,8,4>, <512,8,4> ->
    <256,16,8>; tests/test_search_shapes_cpu.py asserts both sides of the threshold); the tables are the ones of the shape chosen at
    load.  Every utterance must come out as in a batch of three, bit for bit."""
    from rhasspy_speech_amd import synth
    assert ssc.CASES[name]["reg"] in ("<512,4,2>", "<512,8,4>") and (not exact or ssc.CASES[name]["exact_ok"])
    model = _model(files, name, "default", exact_token_order=exact)
    if exact:
        assert "token_order: exact" in model.describe()
    clips = [synth.synth_utterance(400 + i, 8000) for i in range(8)]
    n = _crowded_at()
    big = model.decode_batch([clips[u % 8] for u in range(n)])
    small = {}
    for lo in (0, 3, 5):
        r = model.decode_batch(clips[lo:lo + 3])
        for j in range(3):
            small[lo + j] = (r.words(j), r.costs(j), r.counters(j)[:4], r.counters(j)[5:7])
    assert any(w for w, *_ in small.values())
    for u in range(n):
        assert (big.words(u), big.costs(u), big.counters(u)[:4], big.counters(u)[5:7]) == small[u % 8], u
    model.close()
