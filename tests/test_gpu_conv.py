"""CNN-TDNN models (TimeHeightConvolutionComponent, PermuteComponent) on the GPU, through the C ABI, against what the reference's
decoder binaries gave for the cases of tests/conv_cases.py (tests/golden/conv/, written by tests/gen_conv_golden.py).

Tolerances are test_gpu_fbank.py's: words and 5-best exact; log-likelihoods 1e-4 absolute (the project's bound); costs 2e-3 relative
on the 1-best, rtol 2e-4 + atol 2e-3 on the 5-best.  Every convolution op's output buffer is held to 1e-4 of its row's largest
element in the float64 restatement of conv_cases.py, so that a wrong tile is named by layer."""
import re

import numpy as np
import pytest

from tests import conv_cases as cc

pytestmark = pytest.mark.gpu

LOGLIKE_TOL = 1e-4
LAYER_REL_TOL = 1e-4
IVEC_TOL = 1e-4
DECODED = [n for n in cc.CASES if n not in cc.NO_GOLDEN and n != "cv_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model, pcm): the case's files written and its model loaded once (cases of one model_key share the model)."""
    from rhasspy_speech_amd import _lib
    models, done = {}, {}

    def get(name):
        if name not in done:
            key = cc.model_key(name)
            md, gd, _, pcm = cc.build_case_files(name, tmp_path_factory.mktemp(name))
            if key not in models:
                models[key] = _lib.Model(md, gd, _lib.default_opts(keep_intermediates=1))
            done[name] = (models[key], pcm)
        return done[name]
    return get


@pytest.fixture(scope="module")
def restated():
    """name -> (float64 log-likelihoods, [float64 conv layer outputs]), computed once per case."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = cc.restate(name)
        return done[name]
    return get


def parse_nbest(text: bytes):
    return [[int(x) for x in line.split()[1:]] for line in text.decode().splitlines() if line.split()]


def _check_nbest(res, g, mode):
    ref = parse_nbest(bytes(g[f"{mode}_nbest_text"]))
    got = [res.words(0, k) for k in range(res.num_hyps(0))]
    assert got == ref, (got, ref)
    gc = np.array([res.costs(0, k)[0] for k in range(len(got))])
    ac = np.array([res.costs(0, k)[1] for k in range(len(got))])
    np.testing.assert_allclose(gc, g[f"{mode}_graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(ac, g[f"{mode}_acoustic_cost"], rtol=2e-4, atol=2e-3)
    assert abs(gc[0] - g[f"{mode}_graph_cost"][0]) < 2e-3 * max(1.0, abs(gc[0]))
    assert abs(ac[0] - g[f"{mode}_acoustic_cost"][0]) < 2e-3 * max(1.0, abs(ac[0]))
    assert res.text(0).split() == bytes(g[f"{mode}_nbest_text"]).split()


@pytest.mark.parametrize("name", DECODED)
def test_offline_case(built, restated, name):
    g = cc.load_golden(name)
    model, pcm = built(name)
    res = model.decode_batch([pcm], nbest=cc.NBEST)
    assert res.num_frames(0) == int(g["offline_num_frames"])
    if "offline_ivector" in g.files:
        assert np.abs(res.matrix(0, 1) - g["offline_ivector"]).max() < IVEC_TOL
    # every convolution, in network order, against the restatement evaluated on the golden's input rows (the rows this call computed
    # differ from those by the feature kernels' 2e-4 at most, far inside the bound after a layer's weights)
    layers = restated(name)[1]
    strides = [int(m.group(1)) if m else 1 for m in
               (re.search(r"rows=every-(\d+)", l) for l in model.describe().splitlines() if l.startswith("op: conv "))]
    assert len(layers) == len(cc.conv_geometry(name)) == len(strides)
    for k, want in enumerate(layers):
        got = res.matrix(0, 3 + k)
        assert got.shape == want.shape
        got, want = got[::strides[k]], want[::strides[k]]
        rel = float((np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)).max())
        print(f"{name}: convolution {k + 1} max error relative to the row maximum {rel:.3g}")
        assert rel < LAYER_REL_TOL, (name, k, rel)
    diff = float(np.abs(res.matrix(0, 2) - g["offline_loglikes"]).max())
    print(f"{name}: log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "offline")
    assert model.decode_batch([pcm], nbest=1).words(0) == res.words(0, 0)


@pytest.mark.parametrize("name", DECODED)
def test_streamed_case(built, name):
    """1024-sample ticks, advanced as they arrive: what online2-cli-nnet3-decode-faster reads at a time."""
    from rhasspy_speech_amd import _lib
    g = cc.load_golden(name)
    model, pcm = built(name)
    st = _lib.Stream(model)
    for i in range(0, len(pcm), 1024):
        st.accept(pcm[i:i + 1024])
        st.advance()
    res = st.finish(nbest=cc.NBEST)
    assert res.num_frames(0) == int(g["stream_num_frames"])
    if "stream_ivector" in g.files:
        iv = res.matrix(0, 1)
        assert iv.shape == g["stream_ivector"].shape and np.abs(iv - g["stream_ivector"]).max() < IVEC_TOL
    diff = float(np.abs(res.matrix(0, 2) - g["stream_loglikes"]).max())
    print(f"{name}: streamed log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "stream")


@pytest.mark.parametrize("name", ["cv_basic", "cv_recipe", "cv_wide", "cv_fsf3"])
def test_incremental_stream_equals_batch_replay(built, name, monkeypatch):
    """stream.cc against the batch replay of the same stream (RS_STREAM_BATCH=1): rows, iVectors, log-likelihoods bit for bit -- the
    order of a convolution's sum does not depend on where a frame falls in a tile, a chunk or the batch."""
    from rhasspy_speech_amd import _lib
    model, pcm = built(name)

    def run(advance):
        st = _lib.Stream(model)
        for i in range(0, len(pcm), 2048):
            st.accept(pcm[i:i + 2048])
            if advance:
                st.advance()
        return st.finish(nbest=1)

    inc = run(True)
    monkeypatch.setenv("RS_STREAM_BATCH", "1")
    rep = run(False)
    monkeypatch.delenv("RS_STREAM_BATCH")
    for kind in (0, 1, 2):
        if kind == 1 and name != "cv_recipe":
            continue
        np.testing.assert_array_equal(inc.matrix(0, kind), rep.matrix(0, kind))
    assert inc.words(0) == rep.words(0) and inc.costs(0) == rep.costs(0)


def test_ragged_batch_of_the_cases_that_share_a_model(built):
    """cv_basic, cv_len0 and cv_len1 decode with one model: in one ragged batch (the clip without a frame in the middle, further clips
    of odd lengths around them) every utterance gets its single-utterance result bit for bit, convolution outputs included."""
    from rhasspy_speech_amd import synth
    names = [n for n in cc.CASES if cc.model_key(n) == cc.model_key("cv_basic")]
    assert names == ["cv_basic", "cv_len0", "cv_len1"]
    model = built("cv_basic")[0]
    assert all(built(n)[0] is model for n in names)
    pcms = [built(n)[1] for n in names] + [synth.synth_utterance(80 + i, n) for i, n in enumerate([16001, 560, 8000])]
    batch = model.decode_batch(pcms)
    for i, p in enumerate(pcms):
        single = model.decode_batch([p])
        assert batch.num_frames(i) == single.num_frames(0)
        if single.num_frames(0) == 0:
            continue
        assert batch.words(i) == single.words(0) and batch.costs(i) == single.costs(0)
        for kind in (0, 2, 3, 4, 5):
            np.testing.assert_array_equal(batch.matrix(i, kind), single.matrix(0, kind))


def test_a_clip_without_a_frame_fails_like_the_reference(built):
    """cv_len0: both reference binaries end with GetLattice's error; the result says the same.  cv_len1 (one frame) is among DECODED."""
    from rhasspy_speech_amd import _lib
    g = cc.load_golden("cv_len0")
    assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
    model, pcm = built("cv_len0")
    res = model.decode_batch([pcm])
    assert res.num_frames(0) == 0
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        res.words(0)
    st = _lib.Stream(model)
    st.accept(pcm)
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        st.finish().words(0)
