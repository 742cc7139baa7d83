"""TDNN-attention models (RestrictedAttentionComponent: the layers of xconfig/attention.py) on the GPU, through the C ABI, against what
the reference's decoder binaries gave for the cases of tests/attention_cases.py (tests/golden/attention/, written by
tests/gen_attention_golden.py).  Every one of these fails on the commit before: the load was refused ("component type
RestrictedAttentionComponent ... is not supported by the HIP acoustic-model kernels").

Tolerances are the other model families': words and 5-best exact; log-likelihoods 1e-4 absolute (the project's bound); costs 2e-3
relative on the 1-best, rtol 2e-4 + atol 2e-3 on the 5-best; iVectors 1e-4.  Every attention op's output rows (result matrix kind
128 + k: weighted values and softmax weights, both O(1)) are held to 1e-4 absolute against the float64 restatement of
attention_cases.py, so that a wrong tile or head is named by layer.  The models are loaded with stream_min_ticks = 1: an advance
call per tick really advances, so the three delivery patterns cut the rows into different chunks."""
import re

import numpy as np
import pytest

from tests import attention_cases as ac

pytestmark = pytest.mark.gpu

LOGLIKE_TOL = 1e-4
TAP_TOL = 1e-4
IVEC_TOL = 1e-4
DECODED = [n for n in ac.CASES if n not in ac.NO_GOLDEN and n != "at_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model, pcm): the case's files written and its model loaded once (cases of one model_key share the model)."""
    from rhasspy_speech_amd import _lib
    models, done = {}, {}

    def get(name):
        if name not in done:
            key = ac.model_key(name)
            md, gd, _, pcm = ac.build_case_files(name, tmp_path_factory.mktemp(name))
            if key not in models:
                models[key] = _lib.Model(md, gd, _lib.default_opts(keep_intermediates=1, stream_min_ticks=1))
            done[name] = (models[key], pcm)
        return done[name]
    return get


@pytest.fixture(scope="module")
def restated():
    """name -> (float64 log-likelihoods, [float64 attention outputs], max |b|), computed once per case."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = ac.restate(name)
        return done[name]
    return get


def parse_nbest(text: bytes):
    return [[int(x) for x in line.split()[1:]] for line in text.decode().splitlines() if line.split()]


def _check_nbest(res, g, mode):
    ref = parse_nbest(bytes(g[f"{mode}_nbest_text"]))
    got = [res.words(0, k) for k in range(res.num_hyps(0))]
    assert got == ref, (got, ref)
    gc = np.array([res.costs(0, k)[0] for k in range(len(got))])
    acc = np.array([res.costs(0, k)[1] for k in range(len(got))])
    np.testing.assert_allclose(gc, g[f"{mode}_graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(acc, g[f"{mode}_acoustic_cost"], rtol=2e-4, atol=2e-3)
    assert abs(gc[0] - g[f"{mode}_graph_cost"][0]) < 2e-3 * max(1.0, abs(gc[0]))
    assert abs(acc[0] - g[f"{mode}_acoustic_cost"][0]) < 2e-3 * max(1.0, abs(acc[0]))
    assert res.text(0).split() == bytes(g[f"{mode}_nbest_text"]).split()


def _op_strides(model):
    return [int(m.group(1)) if m else 1 for m in
            (re.search(r"rows=every-(\d+)", l) for l in model.describe().splitlines() if l.startswith("op: attention "))]


@pytest.mark.parametrize("name", DECODED)
def test_offline_case(built, restated, name):
    """Measured on the MI355X when the goldens were made, maxima over the cases: log-likelihoods against the reference 2.4e-05
    (at_sharp, logits up to 146; 5.1e-06 on the others), taps against the float64 restatement 4.3e-05 (at_sharp), 1.6e-05
    (at_recipe_head), 7.5e-06 on the others."""
    g = ac.load_golden(name)
    model, pcm = built(name)
    res = model.decode_batch([pcm], nbest=ac.NBEST)
    assert res.num_frames(0) == int(g["offline_num_frames"])
    if "offline_ivector" in g.files:
        assert np.abs(res.matrix(0, 1) - g["offline_ivector"]).max() < IVEC_TOL
    # every attention op, in network order, against the restatement evaluated on the golden's input rows (the rows this call
    # computed differ from those by the feature kernels' rounding only: dither 0, or the reference's own noise)
    taps = restated(name)[1]
    strides = _op_strides(model)
    assert len(taps) == len(ac.layers_of(name)) == len(strides)
    for k, want in enumerate(taps):
        got = res.matrix(0, 128 + k)
        assert got.shape == want.shape
        got, want = got[::strides[k]], want[::strides[k]]
        assert np.isfinite(got).all()
        diff = float(np.abs(got - want).max())
        print(f"{name}: attention op {k + 1} max abs diff from the float64 restatement {diff:.3g}")
        assert diff < TAP_TOL, (name, k, diff)
    diff = float(np.abs(res.matrix(0, 2) - g["offline_loglikes"]).max())
    print(f"{name}: log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "offline")
    assert model.decode_batch([pcm], nbest=1).words(0) == res.words(0, 0)


def _stream(model, pcm, piece, advance, nbest=1):
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model)
    for i in range(0, len(pcm), piece):
        st.accept(pcm[i:i + piece])
        if advance:
            st.advance()
    return st.finish(nbest=nbest)


@pytest.mark.parametrize("name", DECODED)
def test_streamed_case(built, name):
    """1024-sample ticks, advanced as they arrive (what online2-cli-nnet3-decode-faster reads at a time) against the stream golden;
    2048-sample pieces and everything-then-finish are bit for bit the same rows, words and costs."""
    g = ac.load_golden(name)
    model, pcm = built(name)
    res = _stream(model, pcm, 1024, True, nbest=ac.NBEST)
    assert res.num_frames(0) == int(g["stream_num_frames"])
    if "stream_ivector" in g.files:
        iv = res.matrix(0, 1)
        assert iv.shape == g["stream_ivector"].shape and np.abs(iv - g["stream_ivector"]).max() < IVEC_TOL
    diff = float(np.abs(res.matrix(0, 2) - g["stream_loglikes"]).max())
    print(f"{name}: streamed log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "stream")
    for other in (_stream(model, pcm, 2048, True, nbest=ac.NBEST), _stream(model, pcm, len(pcm), False, nbest=ac.NBEST)):
        for kind in (0, 1, 2) if "stream_ivector" in g.files else (0, 2):
            np.testing.assert_array_equal(other.matrix(0, kind), res.matrix(0, kind))
        assert [other.words(0, k) for k in range(other.num_hyps(0))] == [res.words(0, k) for k in range(res.num_hyps(0))]
        assert [other.costs(0, k) for k in range(other.num_hyps(0))] == [res.costs(0, k) for k in range(res.num_hyps(0))]


@pytest.mark.parametrize("name", ["at_basic", "at_recipe_head", "at_stack", "at_fsf3", "at_fsf3_s2", "at_iv"])
def test_incremental_stream_equals_batch_replay(built, name, monkeypatch):
    """stream.cc against the batch replay of the same stream (RS_STREAM_BATCH=1): rows, iVectors, log-likelihoods bit for bit -- an
    attention row does not depend on the advance it was computed in, nor on where its frame sits in a tile or a run."""
    g = ac.load_golden(name)
    model, pcm = built(name)
    inc = _stream(model, pcm, 2048, True)
    monkeypatch.setenv("RS_STREAM_BATCH", "1")
    rep = _stream(model, pcm, 2048, False)
    monkeypatch.delenv("RS_STREAM_BATCH")
    for kind in (0, 1, 2) if "stream_ivector" in g.files else (0, 2):
        np.testing.assert_array_equal(inc.matrix(0, kind), rep.matrix(0, kind))
    assert inc.words(0) == rep.words(0) and inc.costs(0) == rep.costs(0)


def test_ragged_batch_of_the_cases_that_share_a_model(built):
    """at_basic and the length cases decode with one model: in one ragged batch (the clip without a frame in the middle, three clips
    of odd lengths around them: tiles that hold rows of two utterances) every utterance gets its single-utterance result bit for
    bit, the attention op's rows included."""
    from rhasspy_speech_amd import synth
    names = [n for n in ac.CASES if n not in ac.NO_GOLDEN and ac.model_key(n) == ac.model_key("at_basic")]
    assert names == ["at_basic", "at_len0", "at_len1", "at_len2", "at_lenN"]
    model = built("at_basic")[0]
    assert all(built(n)[0] is model for n in names)
    odd = [synth.synth_utterance(150 + i, n) for i, n in enumerate([16001, 733, 8000])]
    pcms = [odd[0], built("at_basic")[1], built("at_len1")[1], built("at_len0")[1], built("at_len2")[1], odd[1], built("at_lenN")[1], odd[2]]
    batch = model.decode_batch(pcms)
    for i, p in enumerate(pcms):
        single = model.decode_batch([p])
        assert batch.num_frames(i) == single.num_frames(0)
        if single.num_frames(0) == 0:
            continue
        assert batch.words(i) == single.words(0) and batch.costs(i) == single.costs(0)
        for kind in (0, 2, 128):
            np.testing.assert_array_equal(batch.matrix(i, kind), single.matrix(0, kind))


def test_sharp_logits_stay_finite_and_normalised(built, restated):
    """at_sharp: |b| beyond 100 in the restatement (a softmax without the maximum subtracted overflows there); the op's rows are
    finite and every head's softmax weights sum to 1 within 1e-6."""
    assert restated("at_sharp")[2] > 100.0
    model, pcm = built("at_sharp")
    tap = model.decode_batch([pcm]).matrix(0, 128)
    (_, layer), = ac.layers_of("at_sharp")
    C, _, out_dim = ac.synth.attention_layer_dims(layer)
    H, V = int(layer["heads"]), int(layer["value_dim"])
    assert tap.shape[1] == out_dim == H * (V + C) and np.isfinite(tap).all()
    c = tap.reshape(tap.shape[0], H, V + C)[:, :, V:]
    assert (c >= 0.0).all()
    err = float(np.abs(c.astype(np.float64).sum(axis=2) - 1.0).max())
    print(f"at_sharp: max |sum c - 1| {err:.3g}")
    assert err < 1e-6, err


def test_the_tap_is_a_batch_intermediate_only(built):
    """Kind 128 + k: the k-th attention op; one past the last is an unknown kind; a stream result holds none."""
    from rhasspy_speech_amd import _lib
    model, pcm = built("at_stack")
    res = model.decode_batch([pcm])
    assert res.matrix(0, 128).shape[1] == 24 and res.matrix(0, 129).shape[1] == 33
    with pytest.raises(_lib.RsError, match="unknown kind"):
        res.matrix(0, 130)
    with pytest.raises(_lib.RsError, match="unknown kind"):
        _stream(model, pcm, 2048, True).matrix(0, 128)


def test_a_clip_without_a_frame_fails_like_the_reference(built):
    """at_len0: both reference binaries end with GetLattice's error; the result says the same."""
    from rhasspy_speech_amd import _lib
    g = ac.load_golden("at_len0")
    assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
    model, pcm = built("at_len0")
    res = model.decode_batch([pcm])
    assert res.num_frames(0) == 0
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        res.words(0)
    st = _lib.Stream(model)
    st.accept(pcm)
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        st.finish().words(0)
