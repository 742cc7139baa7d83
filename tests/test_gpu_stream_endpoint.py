"""Endpoint detection on streams on the GPU (rs_streams_endpoint / rs_streams_finalize): against the reference's goldens
(online2-wav-nnet3-latgen-faster --online=true --do-endpointing=true --chunk-length=0.064, tools/gen_endpoint_golden.py), against
the sequential oracle on every tick, delivery independence, non-perturbation, batched = single, rows read, streams whose search is
deferred to finish, edge cases, the stream transcriber end to end."""
import asyncio

import numpy as np
import pytest

from tests import cases, endpoint_cases as ec
from tests.test_gpu_stream_partial import COST_ATOL, COST_RTOL, _same_result

pytestmark = pytest.mark.gpu

# n-best costs against the reference's: the tolerance tests/test_gpu_parity.py holds n-best costs to (test_offline_nbest_case)
REF_COST_RTOL, REF_COST_ATOL = 2e-4, 2e-3
TICK = ec.TICK
EARLY = [n for n in ec.ENDPOINT_CASES if (ec.GOLDEN_DIR / f"{n}.json").exists() and ec.load_golden(n)["stopped_early"]]
NEVER = [n for n in ec.ENDPOINT_CASES if (ec.GOLDEN_DIR / f"{n}.json").exists() and not ec.load_golden(n)["stopped_early"]]


@pytest.fixture(scope="module")
def ep_cache(tmp_path_factory):
    """Builds (once per module) the model / graph / wav files of an endpoint case."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = ec.build_files(name, tmp_path_factory.mktemp(name))
        return built[name]

    return get


def _model(ep_cache, name, **extra):
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir, _, pcm = ep_cache(name)
    o = dict(keep_intermediates=1)
    o.update(cases.CASES[ec.ENDPOINT_CASES[name]["base"]].get("opts", {}))
    o.update(extra)
    return _lib.Model(model_dir, graph_dir, _lib.default_opts(**o)), pcm


def _run_ticks(model, pcm, opts=None, partials=False):
    """Feeds the complete 1024-sample ticks of pcm one at a time with an endpoint query after each -> (stream, records)."""
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model)
    recs = []
    for k in range(0, len(pcm) - len(pcm) % TICK, TICK):
        st.accept(pcm[k:k + TICK])
        if partials:
            st.partial().close()
        recs.append(st.endpoint(opts).as_tuple())
    return st, recs


def test_the_set_of_golden_cases_meets_its_conditions():
    assert len(EARLY) + len(NEVER) == len(ec.ENDPOINT_CASES), "a case has no golden"
    assert len(EARLY) >= 8 and len(NEVER) >= 2
    assert len({ec.load_golden(n)["rule"] for n in EARLY}) >= 3
    # at least one early stop comes from a rule whose max-relative-cost is finite (online-endpoint.h:152-157 unless the case sets it),
    # with a finite cost recorded by the reference on that tick
    default_max_cost = {1: np.inf, 2: 2.0, 3: 8.0, 4: np.inf, 5: np.inf}
    finite = []
    for n in EARLY:
        g = ec.load_golden(n)
        bound = float(ec.ENDPOINT_CASES[n]["lines"].get(f"rule{g['rule']}.max-relative-cost", default_max_cost[g["rule"]]))
        if np.isfinite(bound):
            assert g["values"]["relative_cost"] != "inf" and float(g["values"]["relative_cost"]) <= bound, n
            finite.append(n)
    assert finite, "no early stop through a rule with a finite max-relative-cost"


# ---------------------------------------------------------------------------------------------- 1: the reference's goldens
@pytest.mark.parametrize("name", list(ec.ENDPOINT_CASES))
def test_endpoint_and_finalize_against_the_reference(ep_cache, name):
    g = ec.load_golden(name)
    model, pcm = _model(ep_cache, name)
    assert g["lines"] == ec.endpoint_lines(ec.ENDPOINT_CASES[name]) and g["num_chunks"] == (len(pcm) + TICK - 1) // TICK
    st, recs = _run_ticks(model, pcm)
    detecting = [j for j, r in enumerate(recs) if r[0]]
    print(name, "first detections", [(j, recs[j]) for j in detecting[:2]], "golden", g["frames"], g["rule"], g["stop_tick"])
    if not g["stopped_early"]:
        assert [j for j in detecting if j < g["num_chunks"] - 1] == [], "a detection on a tick before the last; the reference has none"
        st.close()
        return
    assert detecting and detecting[0] == g["stop_tick"]
    first = recs[detecting[0]]
    assert first[0] == g["rule"] and first[1] == g["frames"]
    v = g["values"]
    shift = first[4]
    np.testing.assert_allclose(first[2] * shift, v["trailing_silence"], atol=1e-4)
    np.testing.assert_allclose(first[1] * shift, v["utterance_length"], atol=1e-4)
    if v["relative_cost"] == "inf":
        assert np.isinf(first[3])
    else:
        np.testing.assert_allclose(first[3], v["relative_cost"], rtol=1e-3, atol=1e-2)      # (the log prints 6 digits)
    # finalize at the endpoint: a fresh stream fed up to the detecting tick, like the reference breaks out of its chunk loop
    from rhasspy_speech_amd import _lib
    st.close()
    st = _lib.Stream(model)
    for k in range(detecting[0] + 1):
        st.accept(pcm[k * TICK:(k + 1) * TICK])
        assert st.endpoint().detected == (g["rule"] if k == detecting[0] else 0)
    res = st.finalize(nbest=cases.NBEST)
    assert res.num_frames(0) == g["frames"]
    assert [res.words(0, k) for k in range(res.num_hyps(0))] == [h["words"] for h in g["nbest"]]
    for k, h in enumerate(g["nbest"]):
        print(name, k, res.costs(0, k), (h["graph_cost"], h["acoustic_cost"]))
        np.testing.assert_allclose(res.costs(0, k), (h["graph_cost"], h["acoustic_cost"]), rtol=REF_COST_RTOL, atol=REF_COST_ATOL)
    with pytest.raises(_lib.RsError, match="already finished"):
        st.endpoint()
    st.close()


# ---------------------------------------------------------------------------------------------- 2: the oracle, every tick
def _check_against_oracle(ep_cache, name, recs, ll, opts, extra=None, max_checks=None):
    from oracle import pipeline
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir, _, _ = ep_cache(name)
    base = cases.CASES[ec.ENDPOINT_CASES[name]["base"]]
    o = dict(base.get("opts", {}))
    o.update(extra or {})
    orc = pipeline.Oracle(model_dir, graph_dir, **o)
    tick = ec.TickOracle(orc, ec.tid_to_phone(cases.case_spec(base)))
    sil = [int(p) for p in opts.silence_phones.decode().split(":")]
    want_frames = ec.frames_after_ticks(orc, len(recs) * TICK)
    assert [r[1] for r in recs] == want_frames
    assert all(r[4] == np.float32(ec.frame_shift(orc)) for r in recs)
    by_frames = {}
    for r in recs:
        if r[1] in by_frames:
            assert r == by_frames[r[1]]                  # no new frame searched: the same record
        by_frames[r[1]] = r
    frames = sorted(by_frames)
    if max_checks and len(frames) > max_checks:
        frames = [frames[int(i)] for i in np.unique(np.linspace(0, len(frames) - 1, max_checks).round())]
    for n in frames:
        det, _, ts, rel, shift, rows = by_frames[n]
        if n == 0:
            assert (det, ts, rows) == (0, 0, 0) and np.isinf(rel)
            continue
        o_ts, o_rel, margin = tick.values(ll, n, sil)
        print(name, n, "gpu", (det, ts, rel), "oracle", (o_ts, o_rel), "margin", margin)
        assert ts == o_ts, (n, ts, o_ts)
        if np.isinf(o_rel):
            assert np.isinf(rel), (n, rel)
        else:
            np.testing.assert_allclose(rel, o_rel, rtol=COST_RTOL, atol=COST_ATOL, err_msg=f"frames {n}")
        assert det == _lib.endpoint_rule_fired(opts, n, o_ts, shift, o_rel), n
    return len(frames)


@pytest.mark.parametrize("name", list(ec.ENDPOINT_CASES))
def test_every_tick_matches_the_oracle(ep_cache, name):
    model, pcm = _model(ep_cache, name)
    st, recs = _run_ticks(model, pcm)
    res = st.finish()
    checked = _check_against_oracle(ep_cache, name, recs, res.matrix(0, 2), model.endpoint_opts(), max_checks=12 if len(pcm) > 100000 else None)
    assert checked > 3


EXACT_ORDER = [(n, extra) for n in ec.ENDPOINT_CASES for extra in ({}, dict(max_active=150, min_active=100, beam=10.0))
               if ec.ENDPOINT_CASES[n]["base"] in ("zam_u0", "tiny_hmm_u6", "zam_fsf3_u19") and (not extra or ec.ENDPOINT_CASES[n]["base"] == "zam_u0")]


@pytest.mark.parametrize("name,extra", EXACT_ORDER)
def test_every_tick_with_exact_token_order(ep_cache, name, extra):
    model, pcm = _model(ep_cache, name, exact_token_order=1, **extra)
    st, recs = _run_ticks(model, pcm)
    res = st.finish()
    assert "token_order: exact" in model.describe(), model.describe()
    _check_against_oracle(ep_cache, name, recs, res.matrix(0, 2), model.endpoint_opts(), extra=extra)


def test_exact_token_order_cases_exist():
    assert len({ec.ENDPOINT_CASES[n]["base"] for n, _ in EXACT_ORDER}) >= 2


# ---------------------------------------------------------------------------------------------- 3: delivery independence
@pytest.mark.parametrize("name", list(ec.ENDPOINT_CASES)[:6])
def test_records_do_not_depend_on_the_delivery(ep_cache, name):
    from rhasspy_speech_amd import _lib
    model, pcm = _model(ep_cache, name)
    st, recs = _run_ticks(model, pcm)
    st.close()
    rng = np.random.default_rng(len(name))
    st = _lib.Stream(model)
    pos, n_q = 0, 0
    while pos < len(pcm):
        step = int(rng.integers(1, 9001))
        st.accept(pcm[pos:pos + step])
        pos = min(pos + step, len(pcm))
        ticks = pos // TICK
        got = st.endpoint().as_tuple()
        assert got == (recs[ticks - 1] if ticks else (0, 0, 0, float("inf"), recs[0][4], 0)), (pos, ticks)
        n_q += 1
    assert n_q >= 4
    st.close()


# ---------------------------------------------------------------------------------------------- 4: no perturbation
@pytest.mark.parametrize("partials", [False, True])
@pytest.mark.parametrize("name", list(ec.ENDPOINT_CASES)[:5] + list(ec.ENDPOINT_CASES)[-2:])
def test_endpoint_queries_leave_the_stream_alone(ep_cache, name, partials):
    from rhasspy_speech_amd import _lib
    model, pcm = _model(ep_cache, name)
    st, _ = _run_ticks(model, pcm, partials=partials)
    st.accept(pcm[len(pcm) - len(pcm) % TICK:])
    res = st.finish(nbest=cases.NBEST)
    plain = _lib.Stream(model)
    for k in range(0, len(pcm), TICK):
        plain.accept(pcm[k:k + TICK])
        plain.advance()
    _same_result(res, plain.finish(nbest=cases.NBEST), ec.ENDPOINT_CASES[name]["base"])


def test_partials_are_the_same_with_endpoint_queries_in_between(ep_cache):
    from rhasspy_speech_amd import _lib
    name = list(ec.ENDPOINT_CASES)[0]
    model, pcm = _model(ep_cache, name)
    a, b = _lib.Stream(model), _lib.Stream(model)
    for k in range(0, len(pcm), TICK):
        a.accept(pcm[k:k + TICK])
        b.accept(pcm[k:k + TICK])
        a.endpoint()
        ra, rb = a.partial(), b.partial()
        assert (ra.num_frames(0), ra.words(0), ra.costs(0)) == (rb.num_frames(0), rb.words(0), rb.costs(0))
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 5: batched = single
@pytest.mark.parametrize("name", list(ec.ENDPOINT_CASES)[:1] + [n for n in ec.ENDPOINT_CASES if "fsf3" in n][:1] + [n for n in ec.ENDPOINT_CASES if "arpa" in n][:1])
def test_batched_queries_equal_single_ones(ep_cache, name):
    from rhasspy_speech_amd import _lib, synth
    model, _ = _model(ep_cache, name)
    pcms = [synth.synth_utterance(910 + i, n) for i, n in enumerate([16000 * 6, 30000, 16000 * 4, 2000])]
    batch = [_lib.Stream(model) for _ in pcms]
    single = [_lib.Stream(model) for _ in pcms]
    step = 5000
    for k in range(0, max(len(p) for p in pcms), step):
        for s, p in zip(batch + single, pcms + pcms):
            if k < len(p):
                s.accept(p[k:k + step])
        got = _lib.endpoint_streams(batch)
        for i, s in enumerate(single):
            assert got[i].as_tuple() == s.endpoint().as_tuple(), (k, i)
    assert got[3].as_tuple()[:3] == (0, 0, 0) and np.isinf(got[3].final_relative_cost) and got[3].rows_read == 0      # no decoded frame yet
    assert got[0].num_frames_decoded > got[1].num_frames_decoded > 0
    fb = _lib.finalize_streams(batch[:3], nbest=2)
    for i, s in enumerate(single[:3]):
        one = s.finalize(nbest=2)
        assert fb.num_frames(i) == one.num_frames(0) == got[i].num_frames_decoded
        assert [fb.words(i, k) for k in range(fb.num_hyps(i))] == [one.words(0, k) for k in range(one.num_hyps(0))]
        assert fb.costs(i) == one.costs(0)


# ---------------------------------------------------------------------------------------------- 6: rows read
def test_rows_read_are_the_trailing_silence_plus_one(case_cache):
    """The 30 s case: the walk reads the rows of the trailing silence and the one it stops in, however long the stream has grown;
    with every phone in the list it is the whole stream (the walk ends at the start state)."""
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir, _, pcm = case_cache("zam_long30")
    model = _lib.Model(model_dir, graph_dir, _lib.default_opts(keep_intermediates=0))
    spec = cases.case_spec(cases.CASES["zam_long30"])
    few = _lib.default_endpoint_opts("1")
    every = _lib.default_endpoint_opts(":".join(str(p) for p in range(1, spec.num_phones + 1)))
    st = _lib.Stream(model)
    seen = []
    for k in range(0, len(pcm) - len(pcm) % TICK, TICK):
        st.accept(pcm[k:k + TICK])
        a, b = st.endpoint(few), st.endpoint(every)
        if a.num_frames_decoded == 0:
            assert a.rows_read == b.rows_read == 0
            continue
        assert a.rows_read == a.trailing_silence_frames + 1, (k, a)
        assert b.trailing_silence_frames == b.num_frames_decoded and b.rows_read == b.num_frames_decoded + 1, (k, b)
        seen.append((a.num_frames_decoded, a.rows_read))
    st.close()
    assert seen[-1][0] > 2500
    print("rows read with silence = {1}:", sorted({r for _, r in seen}))
    # bounded by the trailing silence, not by the stream's length: in the second half of the stream no query reads half of it
    assert all(r <= n // 2 for n, r in seen if n > 1500), [x for x in seen if x[0] > 1500 and x[1] > x[0] // 2][:5]


# ---------------------------------------------------------------------------------------------- 7: deferred search
@pytest.mark.parametrize("name", [n for n in ec.ENDPOINT_CASES if "arpa" in n][:1] + list(ec.ENDPOINT_CASES)[:2])
def test_endpoint_on_a_search_deferred_to_finish(ep_cache, name, monkeypatch):
    monkeypatch.setenv("RS_DECODER", "sparse")
    model, pcm = _model(ep_cache, name)
    st, recs = _run_ticks(model, pcm)
    res = st.finish(nbest=cases.NBEST)
    assert all(r[5] == (r[1] + 1 if r[1] else 0) for r in recs)      # the deferred search reads every frame
    _check_against_oracle(ep_cache, name, recs, res.matrix(0, 2), model.endpoint_opts())


def test_deferred_and_register_resident_searches_agree(ep_cache, monkeypatch):
    name = list(ec.ENDPOINT_CASES)[0]
    model, pcm = _model(ep_cache, name)
    st, recs = _run_ticks(model, pcm)
    st.close()
    monkeypatch.setenv("RS_DECODER", "dense")
    model2, _ = _model(ep_cache, name)
    st2, recs2 = _run_ticks(model2, pcm)
    st2.close()
    assert [r[:3] for r in recs] == [r[:3] for r in recs2]
    np.testing.assert_allclose([r[3] for r in recs], [r[3] for r in recs2], rtol=COST_RTOL, atol=COST_ATOL)


# ---------------------------------------------------------------------------------------------- 8: edge cases
def test_silence_list_errors_overrides_and_streams_that_are_gone(ep_cache, case_cache, monkeypatch):
    from rhasspy_speech_amd import _lib, synth
    name = EARLY[0]
    g = ec.load_golden(name)
    model, pcm = _model(ep_cache, name)
    st = _lib.Stream(model)
    r = st.endpoint()                                    # before any sample
    assert r.as_tuple()[:3] == (0, 0, 0) and np.isinf(r.final_relative_cost) and r.rows_read == 0
    st.accept(pcm[:(g["stop_tick"] + 1) * TICK])
    assert st.endpoint().detected == g["rule"]
    # the silence list
    with pytest.raises(_lib.RsError, match="Endpointing requires nonempty --endpoint.silence-phones option") as e:
        st.endpoint(_lib.default_endpoint_opts(""))
    assert e.value.status == _lib.RS_ERR_ARG
    for bad in ("1:2:1", "3:3", "1::2", "1:x", ":1", "1:", "1 :2"):
        with pytest.raises(_lib.RsError, match="Bad --silence-phones option in endpointing config: ") as e:
            st.endpoint(_lib.default_endpoint_opts(bad))
        assert e.value.status == _lib.RS_ERR_ARG
    # opts given by the caller win over the model's: the defaults with a phone no path of this graph visits -> no trailing silence
    spec = cases.case_spec(cases.CASES[ec.ENDPOINT_CASES[name]["base"]])
    o = _lib.default_endpoint_opts(str(spec.num_phones + 7))
    r = st.endpoint(o)
    assert r.detected == 0 and r.trailing_silence_frames == 0 and r.rows_read == 1 and r.num_frames_decoded == g["frames"]
    o.rule[4].min_utterance_length = 0.05
    assert st.endpoint(o).detected == 5
    o.rule[0].min_trailing_silence = 0.0
    assert st.endpoint(o).detected == 1
    assert st.endpoint().detected == g["rule"]           # the errors and overrides above left the stream usable and unchanged
    st.finish()
    for call in (st.endpoint, st.finalize):
        with pytest.raises(_lib.RsError, match="already finished"):
            call()
    st.close()
    with pytest.raises(_lib.RsError, match="rs_streams_partial: null stream"):
        st.partial()
    with pytest.raises(_lib.RsError, match="rs_streams_endpoint: null stream"):
        st.endpoint()
    with pytest.raises(_lib.RsError, match="rs_streams_finalize: null stream"):
        st.finalize()
    # finalize without a decoded frame: like the decode of an empty utterance
    empty = _lib.Stream(model)
    empty.accept(pcm[:700])
    res = empty.finalize()
    with pytest.raises(_lib.RsError, match="You cannot get a lattice if you decoded no frames."):
        res.words(0)
    batch_empty = model.decode_batch([pcm[:100]])
    with pytest.raises(_lib.RsError, match="You cannot get a lattice if you decoded no frames."):
        batch_empty.words(0)
    # a poisoned stream (its advance failed: no room in the pool)
    monkeypatch.setenv("RS_STREAM_POOL_ROWS", "8192")
    monkeypatch.setenv("RS_STREAM_INIT_FRAMES", "4096")
    model2, _ = _model(ep_cache, name)
    a, b = _lib.Stream(model2), _lib.Stream(model2)
    a.accept(synth.synth_utterance(77, 16000 * 45))
    b.accept(pcm)
    with pytest.raises(_lib.RsError, match="pool exhausted"):
        _lib.endpoint_streams([a, b])
    for s in (a, b):
        with pytest.raises(_lib.RsError, match="advance that failed"):
            s.endpoint()
        with pytest.raises(_lib.RsError, match="advance that failed"):
            s.finalize()
    a.close()
    b.close()
    # RS_STREAM_BATCH=1 streams are only decoded at finish
    monkeypatch.setenv("RS_STREAM_BATCH", "1")
    c = _lib.Stream(model)
    c.accept(pcm)
    with pytest.raises(_lib.RsError, match="only decoded at finish"):
        c.endpoint()
    c.close()


def test_finalize_ignores_samples_beyond_the_last_complete_tick(ep_cache):
    from rhasspy_speech_amd import _lib
    name = EARLY[0]
    model, pcm = _model(ep_cache, name)
    n = 20 * TICK
    a, b = _lib.Stream(model), _lib.Stream(model)
    a.accept(pcm[:n])
    b.accept(pcm[:n + 1000])
    ra, rb = a.finalize(nbest=cases.NBEST), b.finalize(nbest=cases.NBEST)
    assert ra.num_frames(0) == rb.num_frames(0) > 0 and ra.text(0) == rb.text(0)
    for k in range(ra.num_hyps(0)):
        assert ra.costs(0, k) == rb.costs(0, k)
    np.testing.assert_array_equal(ra.matrix(0, 2), rb.matrix(0, 2))
    # and it is not what finish gives: finish flushes the feature tail
    c = _lib.Stream(model)
    c.accept(pcm[:n])
    assert c.finish().num_frames(0) > ra.num_frames(0)


# ---------------------------------------------------------------------------------------------- 9: the transcriber
def test_transcriber_until_endpoint_end_to_end(ep_cache, tmp_path):
    from rhasspy_speech_amd import _lib
    from rhasspy_speech_amd.meta import int2sym, texts_from_int2sym
    from rhasspy_speech_amd.transcribe_stream import KaldiNnet3StreamTranscriber
    name = EARLY[0]
    g = ec.load_golden(name)
    model_dir, graph_dir, _, pcm = ep_cache(name)
    base = cases.CASES[ec.ENDPOINT_CASES[name]["base"]].get("opts", {})
    tr = KaldiNnet3StreamTranscriber(model_dir, graph_dir, **{k: v for k, v in base.items() if k in ("max_active", "beam")})
    raw = pcm.astype("<i2").tobytes()
    chunks = [raw[k:k + 2 * TICK] for k in range(0, len(raw), 2 * TICK)]
    pulled = []

    async def audio():
        for i, c in enumerate(chunks):
            pulled.append(i)
            yield c

    got = asyncio.run(tr.async_transcribe_until_endpoint(audio(), tmp_path))
    assert tr.last_endpoint_rule == g["rule"]
    assert len(pulled) == g["stop_tick"] + 1 < len(chunks)
    st = _lib.Stream(tr._ensure_loaded())
    for c in chunks[:len(pulled)]:
        st.accept(c)
    by_hand = texts_from_int2sym(int2sym(st.finalize(1, tr.acoustic_scale).text(0, "utt"), tr._words))
    assert got == by_hand and got
    # a case that never detects: the audio ends first and the result is async_transcribe's
    model_dir, graph_dir, _, pcm = ep_cache(NEVER[0])
    tr2 = KaldiNnet3StreamTranscriber(model_dir, graph_dir)
    raw = pcm.astype("<i2").tobytes()
    # (the last chunk is left out: on it the stream may detect where the wav binary, which flushes before its last advance, differs)
    chunks2 = [raw[k:k + 2 * TICK] for k in range(0, len(raw) - 2 * TICK, 2 * TICK)][:-1]

    async def audio2():
        for c in chunks2:
            yield c

    assert asyncio.run(tr2.async_transcribe_until_endpoint(audio2(), tmp_path)) == asyncio.run(tr2.async_transcribe(audio2(), tmp_path))
    assert tr2.last_endpoint_rule == 0
