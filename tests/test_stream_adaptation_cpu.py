"""Speaker adaptation without a device: the oracle's restatement of the state against the reference's goldens, its Scale /
LimitFrames against a direct dense-matrix restatement, the C symbols, and the ctypes array round trip."""
import numpy as np
import pytest

from tests import adaptation_cases as ac, cases

NEW_SYMBOLS = ["rs_adaptation_new", "rs_streams_adaptation", "rs_stream_adaptation", "rs_stream_open_adapted", "rs_adaptation_export",
               "rs_adaptation_import", "rs_adaptation_free"]


def test_every_case_has_a_golden():
    for name, case in ac.ADAPT_CASES.items():
        g = ac.load_golden(name)
        assert len(g["adapted"]) == len(g["fresh"]) == len(case["utts"]) >= 2
        assert case["spec"]["dither"] == 0.0
        assert all(2.0 <= n / 16000.0 <= 3.0 for _, n in case["utts"])
        # the first utterance of a speaker is a fresh one; every later one is told from a fresh one by the golden itself
        assert g["adapted"][0] == g["fresh"][0]
        for a, f in zip(g["adapted"][1:], g["fresh"][1:]):
            assert abs(a["nbest"][0]["acoustic_cost"] - f["nbest"][0]["acoustic_cost"]) >= 100 * (1e-4 + 2e-6 * abs(f["nbest"][0]["acoustic_cost"]))
    assert ac.load_golden("ad_tiny_endpoint")["stop_ticks"][0] is not None


@pytest.mark.parametrize("name", list(ac.ADAPT_CASES))
def test_oracle_against_the_reference(name, tmp_path):
    from oracle import pipeline
    g = ac.load_golden(name)
    model_dir, graph_dir, _, pcms = ac.build_files(name, tmp_path)
    orc = pipeline.Oracle(model_dir, graph_dir)
    ao = ac.AdaptedOracle(orc, model_dir)
    state = ao.fresh()
    for i, pcm in enumerate(pcms):
        tr, state = ao.run(pcm, state, stop_tick=g["stop_ticks"][i], nbest=cases.NBEST)
        ref = g["adapted"][i]
        assert tr.num_frames == ref["frames"]
        assert [p.words for p in tr.nbest] == [h["words"] for h in ref["nbest"]]
        np.testing.assert_allclose([p.graph_cost for p in tr.nbest], [h["graph_cost"] for h in ref["nbest"]], rtol=2e-4, atol=2e-3)
        np.testing.assert_allclose([p.acoustic_cost for p in tr.nbest], [h["acoustic_cost"] for h in ref["nbest"]], rtol=2e-4, atol=2e-3)


def _dense_scale(lin, quad, nf, scale, prior_offset, max_count):
    """OnlineIvectorEstimationStats::Scale on a full matrix (ivector-extractor.cc:671-693)."""
    I = np.eye(len(lin))
    old = nf
    nf, quad, lin = nf * scale, quad * scale, lin * scale
    if max_count == 0.0:
        lin[0] += prior_offset * (1.0 - scale)
        quad = quad + (1.0 - scale) * I
    else:
        old_ps, new_ps = scale * max(old, max_count) / max_count, max(nf, max_count) / max_count
        lin[0] += prior_offset * (new_ps - old_ps)
        quad = quad + (new_ps - old_ps) * I
    return lin, quad, nf


@pytest.mark.parametrize("max_count", [0.0, 100.0])
def test_scale_and_limit_frames_against_dense(max_count):
    rng = np.random.default_rng(5)
    dim, C = 7, 5
    for nf in (3.0, 40.0, 250.0):      # below the limit; above it and below max_count; above both
        a = rng.normal(size=(dim, dim))
        quad = a @ a.T + np.eye(dim)
        lin = rng.normal(size=dim)
        cm = rng.normal(size=2 * (C + 1))
        cm[C], cm[2 * C + 1] = 10.0 * nf, 0.0
        state = dict(ivector_linear=lin.copy(), ivector_quadratic=ac.pack(quad), ivector_count=np.array([nf]), cmvn_ivector=cm.copy(), cmvn_nnet=cm.copy())
        np.testing.assert_array_equal(ac.unpack(ac.pack(quad), dim), quad)
        out = ac.limit_frames(state, 150.0, 0.1, 2.5, max_count)
        target = float(np.float32(150.0) * np.float32(0.1))
        if nf > target:
            l2, q2, n2 = _dense_scale(lin.copy(), quad.copy(), nf, target / nf, 2.5, max_count)
            np.testing.assert_allclose(out["ivector_count"][0], target, rtol=1e-12)
        else:
            l2, q2, n2 = lin, quad, nf
        np.testing.assert_allclose(out["ivector_linear"], l2, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(ac.unpack(out["ivector_quadratic"], dim), q2, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(out["ivector_count"][0], n2, rtol=1e-13)
        want_cm = cm * float(np.float32(np.float32(150.0) / np.float32(cm[C]))) if cm[C] > 150.0 else cm
        np.testing.assert_allclose(out["cmvn_ivector"], want_cm, rtol=1e-13, atol=0)
        np.testing.assert_array_equal(out["cmvn_nnet"], cm)      # never limited
        # the scaled statistics still solve to the same kind of system: symmetric, positive definite
        assert np.all(np.linalg.eigvalsh(ac.unpack(out["ivector_quadratic"], dim)) > 0)


def test_speaker_term_of_the_cmvn_against_the_frame_by_frame_definition():
    """online_cmvn_speaker against SmoothOnlineCmvnStats (online-feature.cc:372-419) written out per frame, and against
    pipeline.online_cmvn where there are no speaker statistics."""
    from oracle import pipeline
    rng = np.random.default_rng(3)
    T, C, W, SF, GF = 90, 4, 40, 15, 10
    feats = rng.normal(size=(T, C)).astype(np.float32)
    gstats = np.zeros((2, C + 1))
    gstats[0, :C], gstats[0, C] = rng.normal(size=C) * 50, 50.0
    np.testing.assert_array_equal(ac.online_cmvn_speaker(feats, gstats, None, W, SF, GF), pipeline.online_cmvn(feats, gstats, W, GF))
    for scount in (7.0, 300.0):      # the speaker count clamp binds / the speaker_frames and window clamps bind
        spk = np.zeros(2 * (C + 1))
        spk[:C], spk[C] = rng.normal(size=C) * scount, scount
        got = ac.online_cmvn_speaker(feats, gstats, spk, W, SF, GF)
        x = feats.astype(np.float64)
        for t in range(T):
            lo = max(0, t + 1 - W)
            s, n = x[lo:t + 1].sum(0), float(t + 1 - lo)
            if n < W:
                k = min(W - n, SF, scount)
                if k > 0:
                    s, n = s + k / scount * spk[:C], n + k / scount * scount
            if n < W:
                k = min(W - n, GF)
                if k > 0:
                    s, n = s + k / 50.0 * gstats[0, :C], n + k
            np.testing.assert_allclose(got[t], feats[t] - s / n, rtol=0, atol=2e-6)


def test_symbols_are_exported():
    from rhasspy_speech_amd import _lib
    lib = _lib.load_library()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(lib, s), s


def test_array_round_trip_without_a_device(tmp_path):
    """rs_adaptation_new / export / import are host code: a model that is loaded but never moved to a device serves them."""
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir, _, _ = ac.build_files("ad_tiny_nnetcmvn", tmp_path)
    try:
        model = _lib.Model(model_dir, graph_dir, _lib.default_opts())
    except _lib.RsError as e:
        if e.status == _lib.RS_ERR_DEVICE:
            pytest.fail(f"loading a model needs a device here: {e}")
        raise
    fresh = _lib.Adaptation(model).arrays()
    dim = len(fresh["ivector_linear"])
    assert dim > 0 and len(fresh["ivector_quadratic"]) == dim * (dim + 1) // 2
    np.testing.assert_array_equal(ac.unpack(fresh["ivector_quadratic"], dim), np.eye(dim))
    assert fresh["ivector_linear"][0] != 0 and not fresh["ivector_linear"][1:].any() and fresh["ivector_count"][0] == 0
    assert len(fresh["cmvn_ivector"]) == len(fresh["cmvn_nnet"]) > 0 and not fresh["cmvn_ivector"].any()
    rng = np.random.default_rng(1)
    arr = {k: np.abs(rng.normal(size=v.shape)) for k, v in fresh.items()}
    back = _lib.Adaptation.from_arrays(model, arr).arrays()
    for k in arr:
        np.testing.assert_array_equal(back[k], arr[k])
    with pytest.raises(_lib.RsError, match="negative"):
        _lib.Adaptation.from_arrays(model, dict(arr, ivector_count=np.array([-1.0])))
    with pytest.raises(_lib.RsError, match="not finite"):
        _lib.Adaptation.from_arrays(model, dict(arr, cmvn_nnet=arr["cmvn_nnet"] * np.inf))
    with pytest.raises(_lib.RsError, match="sizes"):
        _lib.Adaptation.from_arrays(model, dict(arr, cmvn_nnet=arr["cmvn_nnet"][:-2]))
