"""Alignments on the GPU (rs_decode_opts.emit_alignment; rs_result_alignment / rs_result_alignment_text / rs_result_phones)
against the reference's `nbest-to-linear` alignments and `lattice-to-phone-lattice` phone sequences in
tests/golden/alignments.npz (oracle/gen_alignment_golden.py).  Equality is exact, and no case is exempt.

Two routes give an alignment: a 1-best call without a lattice takes it from the search's own traceback on the device (every
finish stage writes the path's arc per frame); every other call takes the best alignment of each word sequence from the lattice
on the host.  Both are held to the same fixtures, and to each other on hypothesis 0."""
import numpy as np
import pytest

from . import cases
from . import endpoint_cases as ec
from . import length_cases as lc
from . import search_shape_cases as ssc
from .test_alignment_cpu import ALI, hyps, phones_read_off, spec_of
from .test_gpu_parity import make_model

pytestmark = pytest.mark.gpu
TICK = 1024


def check(res, u, key, what, hyp0_only=False):
    """Utterance u of `res` against fixture record `key`: every hypothesis the fixture keeps (the big cases keep two)."""
    from rhasspy_speech_amd import _lib
    ali, words, phones = hyps(key, "ali"), hyps(key, "words"), hyps(key, "phones")
    n = 1 if hyp0_only else len(ali)
    assert res.num_hyps(u) >= n, what
    spec = spec_of(key)
    for k in range(n):
        assert res.words(u, k) == words[k], (what, k)
        got = res.alignment(u, k)
        assert got.dtype == np.int32 and len(got) == res.num_frames(u), (what, k)
        diff = np.nonzero(got != np.asarray(ali[k]))[0] if len(got) == len(ali[k]) else None
        assert diff is not None and len(diff) == 0, (what, k, "frames that differ", diff)
        want = phones_read_off(spec, ali[k])
        if want is None:      # (paths of the padded search-shape graphs that SplitToPhones does not split)
            with pytest.raises(_lib.RsError, match="Could not split word into phones correctly"):
                res.phones(u, k)
            continue
        ph, start, length = res.phones(u, k)
        assert ph.tolist() == phones[k], (what, k)
        assert list(zip(ph.tolist(), start.tolist(), length.tolist())) == want, (what, k)
    # the text form: nbest-to-linear's `ark,t:` lines
    lines = res.alignment_text(u, "utt").decode().splitlines()
    assert len(lines) == res.num_hyps(u)
    for k in range(n):
        assert lines[k] == f"utt-{k + 1} " + "".join(f"{t} " for t in ali[k]), (what, k)


# ---------------------------------------------------------------------------------------------- offline
@pytest.mark.parametrize("name", list(cases.CASES))
def test_offline_case(case_cache, name):
    model, pcm = make_model(case_cache, name, emit_alignment=1, keep_intermediates=0)
    one = model.decode_batch([pcm], nbest=1)
    check(one, 0, f"case__{name}__offline", f"{name} device route", hyp0_only=True)
    five = model.decode_batch([pcm], nbest=cases.NBEST)
    check(five, 0, f"case__{name}__offline", f"{name} lattice route")
    assert (one.alignment(0, 0) == five.alignment(0, 0)).all()
    model.close()


# ---------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("mode", ["finish_only", "advance_every_accept", "advance_irregular"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_streaming_case(case_cache, name, mode):
    """The delivery patterns of test_gpu_parity.test_streaming_case; two streams get the same audio, one finished for the
    1-best (the windows' traceback), one for the n-best (the lattice over the retained rows)."""
    from rhasspy_speech_amd import _lib
    model, pcm = make_model(case_cache, name, emit_alignment=1, keep_intermediates=0)
    a, b = _lib.Stream(model), _lib.Stream(model)
    rng = np.random.default_rng(len(name))
    pos, k = 0, 0
    while pos < len(pcm):
        step = 777 if mode != "advance_irregular" else int(rng.integers(1, 9000))
        for st in (a, b):
            st.accept(pcm[pos:pos + step])
        pos += step
        k += 1
        if mode == "advance_every_accept" or (mode == "advance_irregular" and k % 3 == 0):
            a.advance()
            b.advance()
    one, five = a.finish(nbest=1), b.finish(nbest=cases.NBEST)
    check(one, 0, f"case__{name}__stream", f"{name} {mode} device route", hyp0_only=True)
    check(five, 0, f"case__{name}__stream", f"{name} {mode} lattice route")
    assert (one.alignment(0, 0) == five.alignment(0, 0)).all()
    a.close()
    b.close()
    model.close()


# ---------------------------------------------------------------------------------------------- every search
@pytest.fixture(scope="module")
def shape_files(tmp_path_factory):
    from rhasspy_speech_amd import synth
    root = tmp_path_factory.mktemp("alignment_shapes")
    synth.write_model_dir(root / "model", ssc.spec())
    built = {}

    def get(name):
        if name not in built:
            ssc.write_graph(name, root / name)
            built[name] = (root / "model", root / name)
        return built[name]
    return get


SHAPES = sorted({k.split("__")[1] for k in ALI.files if k.startswith("shape__")})
SHAPE_CLIPS = (0, 1)
SEARCHES = [("auto", {}), ("dense", {"RS_DECODER": "dense"}), ("sparse", {"RS_DECODER": "sparse"}), ("hash", {"RS_DECODER": "hash"}),
            ("exact", {"RS_EXACT_ORDER": "1"})]


def test_shape_subset_is_what_the_issue_asks_for():
    rows = [ssc.CASES[n] for n in SHAPES]
    assert {r["reg"] for r in rows} >= {"<512,4,2>", "<256,32,16>", "<512,8,4>", "none"}      # the register shapes, and beyond the register limit
    assert any(r["exact_ok"] for r in rows) and any(r["dl"] != "none" for r in rows)
    assert max(r.get("depth", 1) for r in rows) == max(c.get("depth", 1) for c in ssc.CASES.values())      # the deepest closure


@pytest.mark.parametrize("search,env", SEARCHES, ids=[s for s, _ in SEARCHES])
@pytest.mark.parametrize("name", SHAPES)
def test_every_search_gives_the_fixture_alignment(shape_files, name, search, env, monkeypatch):
    """The searches a caller can ask for (where one does not apply to the graph the planner falls back, as for any call), each
    through its own finish stage: the 1-best of both clips in one batch, offline; then the n-best from the lattice."""
    from rhasspy_speech_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model_dir, graph_dir = shape_files(name)
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(emit_alignment=1))
    clips = [ssc.clips()[c] for c in SHAPE_CLIPS]
    one = model.decode_batch(clips, nbest=1)
    five = model.decode_batch(clips, nbest=ssc.NBEST)
    for u, c in enumerate(SHAPE_CLIPS):
        check(one, u, f"shape__{name}__c{c}__offline", f"{name} {search} clip {c} device route", hyp0_only=True)
        check(five, u, f"shape__{name}__c{c}__offline", f"{name} {search} clip {c} lattice route")
    model.close()


@pytest.mark.parametrize("name", [n for n in SHAPES if n in ssc.STREAM_CASES])
def test_shape_streams(shape_files, name):
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir = shape_files(name)
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(emit_alignment=1))
    for c in SHAPE_CLIPS:
        pcm = ssc.clips()[c]
        for nbest in (1, ssc.NBEST):
            st = _lib.Stream(model)
            for pos in range(0, len(pcm), 3000):
                st.accept(pcm[pos:pos + 3000])
                st.advance()
            check(st.finish(nbest=nbest), 0, f"shape__{name}__c{c}__stream", f"{name} clip {c} nbest {nbest}", hyp0_only=nbest == 1)
            st.close()
    model.close()


# ---------------------------------------------------------------------------------------------- ragged batch
@pytest.mark.parametrize("nbest", [1, cases.NBEST])
def test_ragged_batch_rows_equal_the_utterances_alone(tmp_path, nbest):
    """A 1-frame, a 2-frame, a 3-frame and a 3-second utterance in one batch: the row stride of the [utt][frame] buffer is the
    longest utterance's, the short rows use its first entries only.  Each row is what the utterance gives alone, and the short
    ones are the reference's."""
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir, pcm = lc.build_variant_files("V1", tmp_path)
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(emit_alignment=1))
    ns = [lc.samples("V1", 1), 48000, lc.samples("V1", 2), lc.samples("V1", 3)]
    clips = [pcm[:n] for n in ns]
    batch = model.decode_batch(clips, nbest=nbest)
    for u, n in enumerate(ns):
        alone = model.decode_batch([clips[u]], nbest=nbest)
        assert batch.num_hyps(u) == alone.num_hyps(0) > 0 and batch.num_frames(u) == alone.num_frames(0) == lc.num_frames("V1", n)
        for k in range(alone.num_hyps(0)):
            assert (batch.alignment(u, k) == alone.alignment(0, k)).all() and len(batch.alignment(u, k)) == lc.num_frames("V1", n)
            assert [x.tolist() for x in batch.phones(u, k)] == [x.tolist() for x in alone.phones(0, k)]
        if n != 48000:
            check(batch, u, f"len__V1__n{n}__offline", f"{n} samples in the batch", hyp0_only=nbest == 1)
    model.close()


@pytest.mark.parametrize("T", [1, 2, 3])
def test_shortest_streams(tmp_path, T):
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir, pcm = lc.build_variant_files("V1", tmp_path)
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(emit_alignment=1))
    n = lc.samples("V1", T)
    for nbest in (1, cases.NBEST):
        st = _lib.Stream(model)
        st.accept(pcm[:n])
        check(st.finish(nbest=nbest), 0, f"len__V1__n{n}__stream", f"{n} samples nbest {nbest}", hyp0_only=nbest == 1)
        st.close()
    model.close()


# ---------------------------------------------------------------------------------------------- finalize at an endpoint
EP = sorted({k.split("__")[1] for k in ALI.files if k.startswith("ep__")})


@pytest.mark.parametrize("nbest", [1, cases.NBEST])
@pytest.mark.parametrize("name", EP)
def test_finalize_at_an_endpoint(tmp_path, name, nbest):
    """rs_streams_finalize on the tick the reference detects its endpoint on (tests/golden/endpoint): the alignment covers exactly
    the frames searched and is the one of the reference's lattice over those frames."""
    from rhasspy_speech_amd import _lib
    g = ec.load_golden(name)
    model_dir, graph_dir, _, pcm = ec.build_files(name, tmp_path)
    o = dict(emit_alignment=1)
    o.update(cases.CASES[ec.ENDPOINT_CASES[name]["base"]].get("opts", {}))
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(**o))
    st = _lib.Stream(model)
    for k in range(g["stop_tick"] + 1):
        st.accept(pcm[k * TICK:(k + 1) * TICK])
    res = st.finalize(nbest=nbest)
    assert res.num_frames(0) == g["frames"] == len(res.alignment(0, 0))
    check(res, 0, f"ep__{name}", f"{name} nbest {nbest}", hyp0_only=nbest == 1)
    st.close()
    model.close()


# ---------------------------------------------------------------------------------------------- the option itself
def _snapshot(res, u, lattice):
    out = dict(frames=res.num_frames(u), words=[res.words(u, k) for k in range(res.num_hyps(u))],
               costs=[res.costs(u, k) for k in range(res.num_hyps(u))], counters=res.counters(u), text=res.text(u))
    if lattice:
        out["lattice"] = res.lattice(u)
    return out


@pytest.mark.parametrize("name", ["tiny_u0", "tiny_arpa_prune_u8", "tiny_fsf3_u16"])
def test_option_on_and_off_give_the_same_results(case_cache, name):
    """Words, costs (bit for bit), counters and the lattice's bytes do not depend on the option, offline and streamed; without it
    the three calls are refused with a message that names it."""
    from rhasspy_speech_amd import _lib
    snaps = {}
    for on in (0, 1):
        for lattice in (0, 1):
            model, pcm = make_model(case_cache, name, emit_alignment=on, emit_lattice=lattice, keep_intermediates=0)
            got = []
            for nbest in (1, cases.NBEST):
                res = model.decode_batch([pcm, pcm[:20000]], nbest=nbest)
                got += [_snapshot(res, u, lattice) for u in (0, 1)]
                st = _lib.Stream(model)
                st.accept(pcm)
                sres = st.finish(nbest=nbest)
                got.append(_snapshot(sres, 0, lattice))
                for r in (res, sres):
                    if on:
                        assert len(r.alignment(0, 0)) == r.num_frames(0)
                        continue
                    for call in (lambda: r.alignment(0, 0), lambda: r.alignment_text(0), lambda: r.phones(0, 0)):
                        with pytest.raises(_lib.RsError, match=r"rs_decode_opts\.emit_alignment = 1") as ei:
                            call()
                        assert ei.value.status == _lib.RS_ERR_ARG
                st.close()
            snaps[(on, lattice)] = got
            model.close()
    for lattice in (0, 1):
        assert snaps[(0, lattice)] == snaps[(1, lattice)]


def test_partial_results_carry_no_alignment(case_cache):
    from rhasspy_speech_amd import _lib
    model, pcm = make_model(case_cache, "tiny_u0", emit_alignment=1, keep_intermediates=0)
    st = _lib.Stream(model)
    st.accept(pcm[:20000])
    part = st.partial()
    assert part.num_frames(0) > 0
    for call in (lambda: part.alignment(0, 0), lambda: part.alignment_text(0), lambda: part.phones(0, 0)):
        with pytest.raises(_lib.RsError, match="results of rs_streams_partial carry no alignment") as ei:
            call()
        assert ei.value.status == _lib.RS_ERR_ARG
    st.accept(pcm[20000:])
    res = st.finish(nbest=1)      # the partial in between changes nothing
    check(res, 0, "case__tiny_u0__stream", "after a partial", hyp0_only=True)
    with pytest.raises(_lib.RsError, match="hypothesis index out of range"):
        res.alignment(0, 1)
    st.close()
    model.close()
