"""Partial results of streams on the GPU (rs_streams_partial / rs_stream_partial): the best path over the frames searched so far
without final costs, against the sequential oracle; partials leave the stream's final result untouched; batched = single; the
traceback anchor; streams whose search is deferred to finish; edge cases; the stream transcriber end to end."""
import asyncio

import numpy as np
import pytest

from tests import cases
from tests.test_gpu_parity import IVEC_TOL, LOGLIKE_TOL, load_golden, make_model, parse_nbest

pytestmark = pytest.mark.gpu

COST_RTOL, COST_ATOL = 2e-6, 1e-4          # the exact-order test's tolerance


def _deliver(st, pcm, mode, seed, after):
    """Feeds pcm to st in the stream tests' patterns; after(st) runs after every accept (every) or every third (irregular)."""
    rng = np.random.default_rng(seed)
    pos, k = 0, 0
    while pos < len(pcm):
        step = 777 if mode == "every" else int(rng.integers(1, 9000))
        st.accept(pcm[pos:pos + step])
        pos += step
        k += 1
        if mode == "every" or k % 3 == 0:
            after(st)


def _take(res, u=0):
    return res.num_frames(u), res.words(u), res.costs(u), res.counters(u)


def _run_partials(model, pcm, mode, seed):
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model)
    parts = []

    def after(s):
        r = s.partial()
        assert r.num_utts == 1 and r.num_hyps(0) == 1
        parts.append(_take(r))
        r.close()
    _deliver(st, pcm, mode, seed, after)
    return st, parts


def _oracle_best(orc, ll, n):
    """1-best of the oracle's lattice over the first n frames, every last-frame state final with weight 0 (no final costs)."""
    import copy
    from oracle import pipeline
    opts = dict(orc.opts, lattice_beam=1e9)            # prunes no frontier token; the search's costs do not depend on it
    # (the graph's final weights go, too: with a final state reached, lattice finalisation would give every other last-frame token
    # an infinite extra cost and prune it whatever the beam -- FinalizeDecoding -- and the search never reads them before that)
    fst = copy.copy(orc.fst)
    fst.final = np.full_like(np.asarray(orc.fst.final), np.inf)
    lattice, _ = pipeline.decode(fst, orc.id2pdf, ll[:n], **opts)
    lattice.final = np.where(lattice.state_frame == n, 0.0, np.inf).astype(np.float32)
    return pipeline.lat.nbest(lattice, 1, orc.opts["lattice_beam"], 1.0)[0]


def _check_against_oracle(case_cache, name, parts, ll, extra=None, max_checks=None):
    from oracle import pipeline
    model_dir, graph_dir, _, _ = case_cache(name)
    o = dict(cases.CASES[name].get("opts", {}))
    o.update(extra or {})
    orc = pipeline.Oracle(model_dir, graph_dir, **o)
    by_frames = {}
    for n, words, costs, _ in parts:
        if n in by_frames:                               # no new frame searched: the same path
            assert (words, costs) == by_frames[n], n
        by_frames[n] = (words, costs)
    frames = sorted(by_frames)
    if not frames:                                       # (a short stream delivered in a few large pieces: no partial was asked for)
        return 0
    assert frames[-1] <= ll.shape[0]
    if max_checks and len(frames) > max_checks:
        frames = [frames[int(i)] for i in np.unique(np.linspace(0, len(frames) - 1, max_checks).round())]
    for n in frames:
        words, costs = by_frames[n]
        if n == 0:
            assert words == [] and costs == (0.0, 0.0)
            continue
        best = _oracle_best(orc, ll, n)
        assert words == best.words, (n, words, best.words)
        np.testing.assert_allclose(costs, (best.graph_cost, best.acoustic_cost), rtol=COST_RTOL, atol=COST_ATOL, err_msg=f"frames {n}")
    return len(frames)


def _check_golden(res, name):
    g = load_golden(name)
    assert res.num_frames(0) == int(g["stream_num_frames"])
    if "stream_ivector" in g:
        assert np.abs(res.matrix(0, 1) - g["stream_ivector"]).max() < IVEC_TOL
    sr, sc = g["loglikes_stride"]
    assert np.abs(res.matrix(0, 2)[::sr, ::sc] - g["stream_loglikes"]).max() < LOGLIKE_TOL
    assert [res.words(0, k) for k in range(res.num_hyps(0))] == parse_nbest(bytes(g["stream_nbest_text"]))


def _same_result(a, b, name):
    assert a.num_frames(0) == b.num_frames(0) and a.num_hyps(0) == b.num_hyps(0)
    for k in range(a.num_hyps(0)):
        assert a.words(0, k) == b.words(0, k)
        np.testing.assert_array_equal(a.costs(0, k), b.costs(0, k))
    for kind in (0, 1, 2):
        if kind == 1 and cases.CASES[name]["spec"].get("ivector_dim", 1) == 0:
            continue
        np.testing.assert_array_equal(a.matrix(0, kind), b.matrix(0, kind))
    assert a.text(0) == b.text(0)


# ---------------------------------------------------------------------------------------------- 1 + 2: oracle parity, non-perturbation
@pytest.mark.parametrize("mode", ["every", "irregular"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_partial_matches_the_oracle_and_leaves_the_stream_alone(case_cache, name, mode):
    from rhasspy_speech_amd import _lib
    model, pcm = make_model(case_cache, name)
    st, parts = _run_partials(model, pcm, mode, len(name))
    res = st.finish(nbest=cases.NBEST)
    _check_golden(res, name)
    # the same stream advanced instead: bit for bit the same finish
    plain = _lib.Stream(model)
    _deliver(plain, pcm, mode, len(name), lambda s: s.advance())
    _same_result(res, plain.finish(nbest=cases.NBEST), name)
    _check_against_oracle(case_cache, name, parts, res.matrix(0, 2), max_checks=12 if len(pcm) > 100000 else None)


def test_partials_without_advances_leave_the_stream_alone(case_cache):
    """finish_only delivery (no advance) with partials in between vs. no calls at all."""
    from rhasspy_speech_amd import _lib
    name = "zam_fsf3_u19"
    model, pcm = make_model(case_cache, name)
    st = _lib.Stream(model)
    for k in range(0, len(pcm), 9000):
        st.accept(pcm[k:k + 9000])
        if (k // 9000) % 2:
            st.partial().close()
    res = st.finish(nbest=cases.NBEST)
    plain = _lib.Stream(model)
    plain.accept(pcm)
    _same_result(res, plain.finish(nbest=cases.NBEST), name)
    _check_golden(res, name)


@pytest.mark.parametrize("name,extra", [("zam_u0", {}), ("zam_u0", dict(max_active=150, min_active=100, beam=10.0)), ("tiny_hmm_u6", {}),
                                        ("zam_fsf3_u19", {})])
def test_partial_with_exact_token_order(case_cache, name, extra):
    model, pcm = make_model(case_cache, name, exact_token_order=1, **extra)
    st, parts = _run_partials(model, pcm, "every", 3)
    res = st.finish()
    assert "token_order: exact" in model.describe(), model.describe()
    _check_against_oracle(case_cache, name, parts, res.matrix(0, 2), extra=extra)


# ---------------------------------------------------------------------------------------------- 3: batched = single
@pytest.mark.parametrize("init_frames", [None, "256"])
@pytest.mark.parametrize("name", ["zam_u1", "tiny_fsf3_u16", "tiny_arpa_u7"])
def test_batched_partials_equal_single_ones(case_cache, name, init_frames, monkeypatch):
    from rhasspy_speech_amd import _lib, synth
    if init_frames:
        monkeypatch.setenv("RS_STREAM_INIT_FRAMES", init_frames)      # rows move while the partials go on
    model, _ = make_model(case_cache, name)
    pcms = [synth.synth_utterance(910 + i, n) for i, n in enumerate([16000 * 9, 30000, 16000 * 5, 2000])]
    batch = [_lib.Stream(model) for _ in pcms]
    single = [_lib.Stream(model) for _ in pcms]
    step = 12000
    for k in range(0, max(len(p) for p in pcms), step):
        for s, p in zip(batch + single, pcms + pcms):
            if k < len(p):
                s.accept(p[k:k + step])
        got = _lib.partial_streams(batch)
        for i, s in enumerate(single):
            one = s.partial()
            assert _take(got, i) == _take(one), (k, i)
    fb = _lib.finish_streams(batch)
    for i, s in enumerate(single):
        one = s.finish()
        assert fb.words(i) == one.words(0) and fb.costs(i) == one.costs(0)


# ---------------------------------------------------------------------------------------------- 4: the anchor
@pytest.mark.parametrize("name", ["zam_long30", "zam_fsf3_u19", "tiny_u0"])
def test_anchor_gives_the_full_walks_results_and_reads_fewer_rows(case_cache, name, monkeypatch):
    from rhasspy_speech_amd import _lib
    model, pcm = make_model(case_cache, name, keep_intermediates=0)

    def run():
        st = _lib.Stream(model)
        out = []
        for k in range(0, len(pcm), 16000):      # 1 s rounds
            st.accept(pcm[k:k + 16000])
            r = st.partial()
            out.append(_take(r))
            r.close()
        st.close()
        return out
    anchored = run()
    monkeypatch.setenv("RS_PARTIAL_FULL_WALK", "1")
    full = run()
    assert [a[:3] for a in anchored] == [f[:3] for f in full]
    rows_anchor, rows_full = sum(a[3][0] for a in anchored), sum(f[3][0] for f in full)
    assert rows_full == sum(f[0] + 1 for f in full if f[0] > 0), "a full walk reads every row"
    if name == "zam_long30":
        assert rows_anchor < 0.5 * rows_full, (rows_anchor, rows_full)
    else:
        assert rows_anchor <= rows_full


# ---------------------------------------------------------------------------------------------- 5: deferred search
@pytest.mark.parametrize("name", ["tiny_arpa_u7", "zam_u1"])
def test_partial_on_a_search_deferred_to_finish(case_cache, name, monkeypatch):
    monkeypatch.setenv("RS_DECODER", "sparse")
    model, pcm = make_model(case_cache, name)
    st, parts = _run_partials(model, pcm, "irregular", 11)
    res = st.finish(nbest=cases.NBEST)
    _check_golden(res, name)
    assert all(p[3][0] == (p[0] + 1 if p[0] else 0) for p in parts)
    _check_against_oracle(case_cache, name, parts, res.matrix(0, 2))


# ---------------------------------------------------------------------------------------------- 6: edge cases
def test_partial_before_any_frame_and_on_streams_that_are_gone(case_cache, monkeypatch):
    from rhasspy_speech_amd import _lib, synth
    model, pcm = make_model(case_cache, "tiny_u0")
    st = _lib.Stream(model)
    for chunk in (None, pcm[:500]):
        if chunk is not None:
            st.accept(chunk)
        r = st.partial()
        assert r.num_frames(0) == 0 and r.num_hyps(0) == 1 and r.words(0) == [] and r.costs(0) == (0.0, 0.0)
    st.accept(pcm[500:])
    assert st.partial().num_frames(0) > 0
    st.finish()
    with pytest.raises(_lib.RsError, match="already finished"):
        st.partial()
    st.close()
    with pytest.raises(_lib.RsError):
        st.partial()
    # a poisoned stream (its advance failed: no room in the pool)
    monkeypatch.setenv("RS_STREAM_POOL_ROWS", "8192")
    monkeypatch.setenv("RS_STREAM_INIT_FRAMES", "4096")
    model2, _ = make_model(case_cache, "tiny_u0")
    a, b = _lib.Stream(model2), _lib.Stream(model2)
    a.accept(synth.synth_utterance(77, 16000 * 45))
    b.accept(pcm)
    with pytest.raises(_lib.RsError, match="pool exhausted"):
        _lib.partial_streams([a, b])
    for s in (a, b):
        with pytest.raises(_lib.RsError, match="advance that failed"):
            s.partial()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 7: the transcriber
def test_transcriber_with_partials_end_to_end(case_cache, tmp_path):
    from rhasspy_speech_amd import _lib
    from rhasspy_speech_amd.meta import decode_meta, int2sym
    from rhasspy_speech_amd.transcribe_stream import KaldiNnet3StreamTranscriber
    model_dir, graph_dir, _, pcm = case_cache("zam_u1")
    tr = KaldiNnet3StreamTranscriber(model_dir, graph_dir)
    raw = pcm.astype("<i2").tobytes()
    chunks = [raw[k:k + 3200] for k in range(0, len(raw), 3200)]

    async def audio():
        for c in chunks:
            yield c

    plain = asyncio.run(tr.async_transcribe(audio(), tmp_path))
    seen = []
    got = asyncio.run(tr.async_transcribe_with_partials(audio(), tmp_path, seen.append))
    assert got == plain and seen
    # the same chunks through Stream.partial on the transcriber's model: every reported text is one of them, in order
    st = _lib.Stream(tr._ensure_loaded())
    texts = []
    for c in chunks:
        st.accept(c)
        r = st.partial()
        line = int2sym(r.text(0, "utt"), tr._words).strip().split(maxsplit=1)
        texts.append(decode_meta(line[1]) if len(line) > 1 else "")
    st.close()
    it = iter(texts)
    assert all(any(t == s for t in it) for s in seen), (seen, texts)
    assert seen[-1] == texts[-1]
