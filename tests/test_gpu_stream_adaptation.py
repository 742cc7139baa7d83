"""Speaker adaptation carried from one stream utterance to the next on the GPU (rs_streams_adaptation / rs_stream_open_adapted):
against the reference's goldens (online2-wav-nnet3-latgen-faster --online=true --chunk-length=0.064 with a spk2utt line of several
utterances, tools/gen_adaptation_golden.py), against the oracle's restatement of the state (tests/adaptation_cases.py), the fresh
state, export / import, batched = single, delivery independence, refusals, the continuous transcriber."""
import asyncio
import ctypes as C

import numpy as np
import pytest

from tests import adaptation_cases as ac, cases

pytestmark = pytest.mark.gpu

TICK = ac.TICK
# n-best costs against the reference's
COST_ATOL, COST_RTOL = 1e-4, 2e-6
NAMES = list(ac.ADAPT_CASES)


@pytest.fixture(scope="module")
def ad_cache(tmp_path_factory):
    """Builds (once per module) the files of a case, loads its model and runs its utterances in order, each opened with the state
    of the ones before: -> dict(model, model_dir, graph_dir, pcms, golden, results, states, feats)."""
    built = {}

    def get(name):
        if name not in built:
            from rhasspy_speech_amd import _lib
            model_dir, graph_dir, _, pcms = ac.build_files(name, tmp_path_factory.mktemp(name))
            model = _lib.Model(model_dir, graph_dir, _lib.default_opts(keep_intermediates=1))
            b = dict(model=model, model_dir=model_dir, graph_dir=graph_dir, pcms=pcms, golden=ac.load_golden(name), results=[], states=[], stops=[])
            ep = model.endpoint_opts() if ac.ADAPT_CASES[name]["endpoint"] else None
            state = None
            for pcm in pcms:
                res, state, stop = _run_ticks(model, pcm, state, ep)
                b["results"].append(res)
                b["states"].append(state)
                b["stops"].append(stop)
            built[name] = b
        return built[name]

    return get


def _run_ticks(model, pcm, state, endpoint_opts=None):
    """One utterance tick by tick (an endpoint query after every tick where the case has rules) -> (result, state after, stop tick)."""
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model, adaptation=state)
    n_ticks = len(pcm) // TICK
    for j in range(n_ticks):
        st.accept(pcm[j * TICK:(j + 1) * TICK])
        if endpoint_opts is not None:
            if st.endpoint(endpoint_opts).detected:
                res = st.finalize(nbest=cases.NBEST)
                return res, st.adaptation(), j
        else:
            st.advance()
    st.accept(pcm[n_ticks * TICK:])
    res = st.finish(nbest=cases.NBEST)
    return res, st.adaptation(), None


def _run(model, pcm, state, pieces=None):
    """One utterance delivered in `pieces` (None: whole) -> (result, state after)."""
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model, adaptation=state)
    k = 0
    for n in (pieces or [len(pcm)]):
        st.accept(pcm[k:k + n])
        st.advance()
        k += n
    st.accept(pcm[k:])
    res = st.finish(nbest=cases.NBEST)
    return res, st.adaptation()


def _same_bits(a, b):
    assert a.num_frames(0) == b.num_frames(0) and a.text(0) == b.text(0)
    for k in range(a.num_hyps(0)):
        assert a.costs(0, k) == b.costs(0, k)
    np.testing.assert_array_equal(a.matrix(0, 2), b.matrix(0, 2))


def _same_state(a, b):
    x, y = a.arrays(), b.arrays()
    for k in x:
        np.testing.assert_array_equal(x[k], y[k], err_msg=k)


# ---------------------------------------------------------------------------------------------- 1: the reference's goldens
@pytest.mark.parametrize("name", NAMES)
def test_against_the_reference(ad_cache, name):
    b = ad_cache(name)
    g = b["golden"]
    assert b["stops"] == g["stop_ticks"]
    if ac.ADAPT_CASES[name]["endpoint"]:
        assert g["stop_ticks"][0] is not None      # (utterance 1 ended through Stream.endpoint() / finalize())
    for i, (res, ref) in enumerate(zip(b["results"], g["adapted"])):
        assert res.num_frames(0) == ref["frames"], i
        assert res.num_hyps(0) == len(ref["nbest"])
        for k, h in enumerate(ref["nbest"]):
            assert res.words(0, k) == h["words"], (i, k)
            got = res.costs(0, k)
            print(f"{name} u{i + 1} hyp {k}: graph {got[0]:.6f} ref {h['graph_cost']:.6f}  acoustic {got[1]:.6f} ref {h['acoustic_cost']:.6f}  "
                  f"diff {got[0] - h['graph_cost']:+.2e} {got[1] - h['acoustic_cost']:+.2e}")
    for i, (res, ref) in enumerate(zip(b["results"], g["adapted"])):
        for k, h in enumerate(ref["nbest"]):
            np.testing.assert_allclose(res.costs(0, k), (h["graph_cost"], h["acoustic_cost"]), rtol=COST_RTOL, atol=COST_ATOL, err_msg=f"u{i + 1} hyp {k}")


# ---------------------------------------------------------------------------------------------- 2: the oracle
def _limits(ao, orc):
    mrf = ao.max_remembered_frames
    return mrf, mrf * orc.ie["posterior_scale"] if orc.ie is not None else None


@pytest.mark.parametrize("name", NAMES)
def test_against_the_oracle(ad_cache, name):
    from oracle import pipeline
    from rhasspy_speech_amd import _lib
    b = ad_cache(name)
    model = b["model"]
    orc = pipeline.Oracle(b["model_dir"], b["graph_dir"])
    ao = ac.AdaptedOracle(orc, b["model_dir"])
    C = orc.mfcc.o.num_ceps
    mrf, target = _limits(ao, orc)
    state = ao.fresh()
    prev = {k: np.zeros_like(v) for k, v in b["states"][0].arrays().items()}
    for i, pcm in enumerate(b["pcms"]):
        tr, state = ao.run(pcm, state, stop_tick=b["stops"][i])
        res, got = b["results"][i], b["states"][i].arrays()
        if i > 0:
            if tr.ivector is not None:
                iv = res.matrix(0, 1)
                assert iv.shape == tr.ivector.shape
                print(f"{name} u{i + 1}: iVector max|diff| {np.abs(iv - tr.ivector).max():.2e}  loglike max|diff| {np.abs(res.matrix(0, 2) - tr.loglikes).max():.2e}")
                np.testing.assert_allclose(iv, tr.ivector, rtol=0, atol=1e-4)
            np.testing.assert_allclose(res.matrix(0, 2), tr.loglikes, rtol=0, atol=1e-4)
        # ---- the exported speaker CMVN blocks = float64 sums of the utterance's raw MFCC rows on top of the carried block, limited
        if orc.nnet_cmvn is None:
            feats = res.matrix(0, 0)      # (no nnet-input CMVN: the result's feature matrix is the raw MFCCs)
            if b["stops"][i] is not None:
                # a finalized stream's result holds the rows searched; GetState covers every frame of the complete ticks: the same
                # samples through a stream that is finished give them all (no dither: a frame does not depend on what follows it)
                n = TICK * (b["stops"][i] + 1)
                full, _ = _run(model, pcm[:n], None)
                feats = full.matrix(0, 0)
                assert feats.shape[0] == orc.mfcc.num_frames(n)
            want = ac.accumulate_cmvn(prev["cmvn_ivector"], feats)
            if want[C] > mrf:
                want = want * (mrf / want[C])
                np.testing.assert_allclose(got["cmvn_ivector"][C], mrf, rtol=1e-9, atol=0)
            np.testing.assert_allclose(got["cmvn_ivector"], want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
        else:
            # (the result's feature matrix is the CMVN'd nnet input there; the nnet-input block is never limited, so its growth IS the
            # utterance's sums: the iVector branch's block is the carried one plus that growth, limited)
            grown = got["cmvn_nnet"] - prev["cmvn_nnet"]
            assert grown[C] == orc.mfcc.num_frames(len(pcm)) and got["cmvn_nnet"][C] == sum(orc.mfcc.num_frames(len(p)) for p in b["pcms"][:i + 1])
            want = prev["cmvn_ivector"] + grown
            if want[C] > mrf:
                want = want * (mrf / want[C])
                np.testing.assert_allclose(got["cmvn_ivector"][C], mrf, rtol=1e-9, atol=0)
            np.testing.assert_allclose(got["cmvn_ivector"], want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
        # ---- the estimator's count where LimitFrames binds (the oracle's statistics before the limit say whether it does)
        if orc.ie is not None:
            target32 = float(np.float32(np.float32(mrf) * np.float32(orc.ie["posterior_scale"])))      # (the reference's BaseFloat product)
            if np.isclose(state["ivector_count"][0], target32, rtol=1e-12, atol=0):
                np.testing.assert_allclose(got["ivector_count"][0], target, rtol=1e-9, atol=0)
        prev = got


# ---------------------------------------------------------------------------------------------- 3: the fresh state
def test_a_fresh_state_is_a_plain_open(ad_cache):
    from rhasspy_speech_amd import _lib
    b = ad_cache("ad_tiny_nnetcmvn")
    model, pcm = b["model"], b["pcms"][0]
    plain, _ = _run(model, pcm, None)
    fresh, _ = _run(model, pcm, _lib.Adaptation(model))
    _same_bits(plain, fresh)
    # state == NULL through rs_stream_open_adapted itself
    h = C.c_void_p()
    _lib._check(_lib.lib().rs_stream_open_adapted(model._h, None, C.byref(h)))
    st = _lib.Stream.__new__(_lib.Stream)
    st.model, st._h = model, h
    st.accept(pcm)
    _same_bits(plain, st.finish(nbest=cases.NBEST))
    # ... and the first utterance of the cached chain was opened without a state
    _same_bits(plain, b["results"][0])


# ---------------------------------------------------------------------------------------------- 4: export -> import -> open
def test_round_trip(ad_cache):
    from rhasspy_speech_amd import _lib
    b = ad_cache("ad_tiny_nnetcmvn")
    model, state = b["model"], b["states"][0]
    again = _lib.Adaptation.from_arrays(model, state.arrays())
    _same_state(state, again)
    ra, sa = _run(model, b["pcms"][1], state)
    rb, sb = _run(model, b["pcms"][1], again)
    _same_bits(ra, rb)
    _same_state(sa, sb)
    _same_bits(ra, b["results"][1])      # (and a state may open any number of streams)


# ---------------------------------------------------------------------------------------------- 5: batched = single
def test_eight_streams_in_one_call(ad_cache):
    from rhasspy_speech_amd import _lib, synth
    b = ad_cache("ad_tiny_3utt")
    model = b["model"]
    s1, s2, s3 = b["states"]
    carried = [s1, s2, None, s3, s2, _lib.Adaptation(model), s1, s3]
    pcms = [synth.synth_utterance(200 + i, n) for i, n in enumerate([30000, 41111, 26000, 48000, 33333, 29000, 44000, 36001])]
    alone = [_run(model, pcm, st, pieces=[TICK] * (len(pcm) // TICK)) for pcm, st in zip(pcms, carried)]
    streams = [_lib.Stream(model, adaptation=st) for st in carried]
    for j in range(max(len(p) for p in pcms) // TICK + 1):
        live = [(s, p[j * TICK:(j + 1) * TICK]) for s, p in zip(streams, pcms) if len(p) > j * TICK]
        if live:
            _lib.accept_streams([s for s, _ in live], [c for _, c in live])
            _lib.advance_streams([s for s, _ in live])
    res = _lib.finish_streams(streams, nbest=cases.NBEST)
    states = _lib.adaptation_of_streams(streams)
    for i, (ra, sa) in enumerate(alone):
        assert res.num_frames(i) == ra.num_frames(0) and res.text(i) == ra.text(0)
        for k in range(ra.num_hyps(0)):
            assert res.costs(i, k) == ra.costs(0, k)
        np.testing.assert_array_equal(res.matrix(i, 2), ra.matrix(0, 2))
        _same_state(states[i], sa)
        _same_state(states[i], streams[i].adaptation())      # one call over the eight = eight single calls


# ---------------------------------------------------------------------------------------------- 6: delivery
def test_delivery_does_not_matter(ad_cache):
    b = ad_cache("ad_tiny_cmvnwin")
    model, pcm, state = b["model"], b["pcms"][1], b["states"][0]
    whole, s_whole = _run(model, pcm, state)
    odd, s_odd = _run(model, pcm, state, pieces=[1000, 3001, 777, 16385, 5, 9000])
    _same_bits(whole, odd)
    _same_state(s_whole, s_odd)
    _same_bits(whole, b["results"][1])      # tick by tick
    _same_state(s_whole, b["states"][1])


# ---------------------------------------------------------------------------------------------- 7: refusals
def test_refusals(ad_cache, monkeypatch, tmp_path):
    from rhasspy_speech_amd import _lib, synth
    b = ad_cache("ad_tiny_3utt")
    model, pcm, state = b["model"], b["pcms"][0], b["states"][0]
    # a stream that has not ended
    st = _lib.Stream(model, adaptation=state)
    st.accept(pcm[:20000])
    st.advance()
    with pytest.raises(_lib.RsError, match="has not ended") as e:
        st.adaptation()
    assert e.value.status == _lib.RS_ERR_ARG
    other = _lib.Stream(model)
    other.accept(pcm)
    other.finish().close()
    with pytest.raises(_lib.RsError, match="has not ended"):
        _lib.adaptation_of_streams([other, st])
    other.adaptation().close()                       # (the ended one of the refused call still gives its state)
    st.accept(pcm[20000:])
    _same_bits(st.finish(nbest=cases.NBEST), _run(model, pcm, state)[0])
    # a state of another model
    nn = ad_cache("ad_tiny_nnetcmvn")
    with pytest.raises(_lib.RsError, match="nnet-input CMVN") as e:
        _lib.Stream(model, adaptation=nn["states"][0])
    assert e.value.status == _lib.RS_ERR_ARG
    arr = state.arrays()
    with pytest.raises(_lib.RsError, match="sizes"):
        _lib.Adaptation.from_arrays(model, dict(arr, ivector_linear=arr["ivector_linear"][:-1]))
    # imported arrays with a negative count or a value that is not finite
    for key, idx, bad, msg in (("ivector_count", 0, -1.0, "negative"), ("cmvn_ivector", len(arr["cmvn_ivector"]) // 2 - 1, -2.0, "negative"),
                               ("ivector_quadratic", 3, float("nan"), "not finite"), ("cmvn_ivector", 1, float("inf"), "not finite")):
        a2 = {k: v.copy() for k, v in arr.items()}
        a2[key][idx] = bad
        with pytest.raises(_lib.RsError, match=msg) as e:
            _lib.Adaptation.from_arrays(model, a2)
        assert e.value.status == _lib.RS_ERR_ARG
    # a failed stream (its advance failed: no room in the pool)
    monkeypatch.setenv("RS_STREAM_POOL_ROWS", "8192")
    monkeypatch.setenv("RS_STREAM_INIT_FRAMES", "4096")
    model2 = _lib.Model(b["model_dir"], b["graph_dir"], _lib.default_opts(keep_intermediates=1))
    x, y = _lib.Stream(model2), _lib.Stream(model2)
    x.accept(synth.synth_utterance(77, 16000 * 45))
    y.accept(pcm)
    with pytest.raises(_lib.RsError, match="pool exhausted"):
        _lib.advance_streams([x, y])
    for s in (x, y):
        with pytest.raises(_lib.RsError, match="advance that failed") as e:
            s.adaptation()
        assert e.value.status == _lib.RS_ERR_ARG
    x.close()
    y.close()
    monkeypatch.delenv("RS_STREAM_POOL_ROWS")
    monkeypatch.delenv("RS_STREAM_INIT_FRAMES")
    # an ended stream whose slot the pool has needed since
    monkeypatch.setenv("RS_STREAM_SLOTS", "2")
    model4 = _lib.Model(b["model_dir"], b["graph_dir"], _lib.default_opts(keep_intermediates=1))
    first = _lib.Stream(model4)
    first.accept(pcm)
    first.finish().close()
    first.adaptation().close()
    second, third = _lib.Stream(model4), _lib.Stream(model4)
    with pytest.raises(_lib.RsError, match="its state is gone") as e:
        first.adaptation()
    assert e.value.status == _lib.RS_ERR_ARG
    third.accept(pcm)
    _same_bits(third.finish(nbest=cases.NBEST), b["results"][0])
    for s in (first, second, third):
        s.close()
    monkeypatch.delenv("RS_STREAM_SLOTS")
    # RS_STREAM_BATCH=1 streams have no state
    monkeypatch.setenv("RS_STREAM_BATCH", "1")
    c = _lib.Stream(model)
    c.accept(pcm)
    c.finish().close()
    with pytest.raises(_lib.RsError, match="RS_STREAM_BATCH=1") as e:
        c.adaptation()
    assert e.value.status == _lib.RS_ERR_ARG
    with pytest.raises(_lib.RsError, match="RS_STREAM_BATCH=1"):
        _lib.Stream(model, adaptation=state)
    monkeypatch.delenv("RS_STREAM_BATCH")
    # the model still works
    _same_bits(_run(model, b["pcms"][1], state)[0], b["results"][1])
    # a model without an extractor and without nnet-input CMVN: the state is empty, opening with it is a plain open
    spec = dict(spec=dict(ivector_dim=0, dither=0.0), graph="grammar", audio="zeros:0")
    model_dir, graph_dir, _, _ = cases.build_case_files(spec, tmp_path)
    m3 = _lib.Model(model_dir, graph_dir, _lib.default_opts(keep_intermediates=1))
    r0, s0 = _run(m3, pcm, None)
    assert all(v.size == 0 for v in s0.arrays().values())
    _same_bits(r0, _run(m3, pcm, s0)[0])
    with pytest.raises(_lib.RsError, match="iVector dimension"):
        _lib.Stream(m3, adaptation=state)


# ---------------------------------------------------------------------------------------------- 8: the transcriber
def test_transcribe_continuous(ad_cache, tmp_path):
    from rhasspy_speech_amd import _lib
    from rhasspy_speech_amd.meta import int2sym, texts_from_int2sym
    from rhasspy_speech_amd.transcribe_stream import KaldiNnet3StreamTranscriber
    b = ad_cache("ad_tiny_endpoint")
    # three utterances, each with a tail of near-silence, in one stream of audio; rule5 cuts it by length
    tails = [np.round(p[:8000].astype(np.float64) * 0.002).astype(np.int16) for p in b["pcms"]]
    audio_pcm = np.concatenate([x for p, t in zip(b["pcms"], tails) for x in (p, t)])
    raw = audio_pcm.astype("<i2").tobytes()
    tr = KaldiNnet3StreamTranscriber(b["model_dir"], b["graph_dir"])

    async def audio():
        for k in range(0, len(raw), 3000):      # (chunks that are no multiple of a tick)
            yield raw[k:k + 3000]

    async def collect():
        return [t async for t in tr.async_transcribe_continuous(audio(), tmp_path)]

    got = asyncio.run(collect())
    # the same by hand: tick by tick, an endpoint query after each, finalize, take the state, open the next utterance with it
    model = tr._ensure_loaded()
    want, state, st, fed = [], None, _lib.Stream(model), 0
    for k in range(0, len(audio_pcm) - len(audio_pcm) % TICK, TICK):
        st.accept(audio_pcm[k:k + TICK])
        fed += TICK
        if st.endpoint().detected:
            want.append(texts_from_int2sym(int2sym(st.finalize(1, tr.acoustic_scale).text(0, "utt"), tr._words)))
            state = st.adaptation()
            st, fed = _lib.Stream(model, adaptation=state), 0
    st.accept(audio_pcm[len(audio_pcm) - len(audio_pcm) % TICK:])
    want.append(texts_from_int2sym(int2sym(st.finish(1, tr.acoustic_scale).text(0, "utt"), tr._words)))
    assert got == want and len(got) >= 3
    _same_state(tr.last_adaptation, st.adaptation())
