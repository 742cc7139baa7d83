"""TDNN-GRU models whose cell is spelled out as separate components (gru-layer / pgru-layer / norm-pgru-layer / opgru-layer /
norm-opgru-layer: PgrucKernel and GrucKernel of nnet_gruc.hip) on the GPU, through the C ABI, against what the reference's decoder
binaries gave for the cases of tests/gruc_cases.py (tests/golden/gruc/, written by tests/gen_gruc_golden.py).  Every one of these
fails on the commit before: the load was refused.

Tolerances are the other model families': words and 5-best exact; log-likelihoods 1e-4 absolute (the project's bound); costs 2e-3
relative on the 1-best, rtol 2e-4 + atol 2e-3 on the 5-best; iVectors 1e-4.  Every block's output rows (result matrix kind 64 + k)
are held to 1e-4 of their row's largest element in the float64 restatement of gruc_cases.py, so that a wrong step is named by block.
The models are loaded with stream_min_ticks = 1: an advance call per tick really advances, so the three delivery patterns re-enter
the blocks at different frames."""
import re

import numpy as np
import pytest

from tests import gruc_cases as lc

pytestmark = pytest.mark.gpu

LOGLIKE_TOL = 1e-4
LAYER_REL_TOL = 1e-4
IVEC_TOL = 1e-4
DECODED = [n for n in lc.CASES if n not in lc.NO_GOLDEN and n != "gc_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model, pcm): the case's files written and its model loaded once (cases of one model_key share the model)."""
    from rhasspy_speech_amd import _lib
    models, done = {}, {}

    def get(name):
        if name not in done:
            key = lc.model_key(name)
            md, gd, _, pcm = lc.build_case_files(name, tmp_path_factory.mktemp(name))
            if key not in models:
                models[key] = _lib.Model(md, gd, _lib.default_opts(keep_intermediates=1, stream_min_ticks=1))
            done[name] = (models[key], pcm)
        return done[name]
    return get


@pytest.fixture(scope="module")
def restated():
    """name -> (float64 log-likelihoods, [float64 block outputs]), computed once per case."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = lc.restate(name)
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


def _block_strides(model):
    return [int(m.group(1)) if m else 1 for m in
            (re.search(r"rows=every-(\d+)", l) for l in model.describe().splitlines() if l.startswith(("op: lstm ", "op: gru ", "op: pgru ")))]


@pytest.mark.parametrize("name", DECODED)
def test_offline_case(built, restated, name):
    g = lc.load_golden(name)
    model, pcm = built(name)
    res = model.decode_batch([pcm], nbest=lc.NBEST)
    assert res.num_frames(0) == int(g["offline_num_frames"])
    if "offline_ivector" in g.files:
        assert np.abs(res.matrix(0, 1) - g["offline_ivector"]).max() < IVEC_TOL
    # every block, in network order, against the restatement evaluated on the golden's input rows (the rows this call computed
    # differ from those by the feature kernels' 2e-4 at most, far inside the bound after a layer's weights)
    blocks = restated(name)[1]
    strides = _block_strides(model)
    assert len(blocks) == len(lc.block_dims(name)) == len(strides)
    for k, want in enumerate(blocks):
        got = res.matrix(0, 64 + k)
        assert got.shape == want.shape
        got, want = got[::strides[k]], want[::strides[k]]
        rel = float((np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)).max())
        print(f"{name}: block {k + 1} max error relative to the row maximum {rel:.3g}")
        assert rel < LAYER_REL_TOL, (name, k, rel)
    diff = float(np.abs(res.matrix(0, 2) - g["offline_loglikes"]).max())
    print(f"{name}: log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "offline")
    assert model.decode_batch([pcm], nbest=1).words(0) == res.words(0, 0)
    # the stacked layer GEMM over the three affines' feed-forward columns in front of every composed block was launched as one
    launched = [l.split()[1] for l in model.describe().splitlines() if l.startswith("gemm_launch: ")]
    for kind, k, _i, _o, layer in lc.block_dims(name):
        if kind != "lstm" and lc.is_composed(layer):
            assert f"{kind}{k}.y_t.x" in launched, launched


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
    g = lc.load_golden(name)
    model, pcm = built(name)
    res = _stream(model, pcm, 1024, True, nbest=lc.NBEST)
    assert res.num_frames(0) == int(g["stream_num_frames"])
    if "stream_ivector" in g.files:
        iv = res.matrix(0, 1)
        assert iv.shape == g["stream_ivector"].shape and np.abs(iv - g["stream_ivector"]).max() < IVEC_TOL
    diff = float(np.abs(res.matrix(0, 2) - g["stream_loglikes"]).max())
    print(f"{name}: streamed log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "stream")
    for other in (_stream(model, pcm, 2048, True, nbest=lc.NBEST), _stream(model, pcm, len(pcm), False, nbest=lc.NBEST)):
        for kind in (0, 1, 2) if "stream_ivector" in g.files else (0, 2):
            np.testing.assert_array_equal(other.matrix(0, kind), res.matrix(0, kind))
        assert [other.words(0, k) for k in range(other.num_hyps(0))] == [res.words(0, k) for k in range(res.num_hyps(0))]
        assert [other.costs(0, k) for k in range(other.num_hyps(0))] == [res.costs(0, k) for k in range(res.num_hyps(0))]


@pytest.mark.parametrize("name", ["gc_pgru", "gc_gru", "gc_npgru", "gc_stack", "gc_fsf3", "gc_opgru_d8"])
def test_incremental_stream_equals_batch_replay(built, name, monkeypatch):
    """stream.cc against the batch replay of the same stream (RS_STREAM_BATCH=1): rows, iVectors, log-likelihoods bit for bit -- a
    block's row does not depend on the advance it was computed in, nor on where its chain sits in a workgroup."""
    g = lc.load_golden(name)
    model, pcm = built(name)
    inc = _stream(model, pcm, 2048, True)
    monkeypatch.setenv("RS_STREAM_BATCH", "1")
    rep = _stream(model, pcm, 2048, False)
    monkeypatch.delenv("RS_STREAM_BATCH")
    for kind in (0, 1, 2) if "stream_ivector" in g.files else (0, 2):
        np.testing.assert_array_equal(inc.matrix(0, kind), rep.matrix(0, kind))
    assert inc.words(0) == rep.words(0) and inc.costs(0) == rep.costs(0)


def test_ragged_batch_of_the_length_cases(built):
    """gc_pgru and the length cases decode with one model: in one ragged batch (the clip without a frame in the middle, three clips
    of odd lengths around them: nine utterances of three chains each, a second workgroup with a partly filled chain tile) every
    utterance gets its single-utterance result bit for bit, block outputs included."""
    from rhasspy_speech_amd import synth
    names = [n for n in lc.CASES if n not in lc.NO_GOLDEN and lc.model_key(n) == lc.model_key("gc_pgru")]
    assert names == ["gc_pgru", "gc_len0", "gc_len1", "gc_len2", "gc_len25", "gc_len47"]
    model = built("gc_pgru")[0]
    assert all(built(n)[0] is model for n in names)
    odd = [synth.synth_utterance(90 + i, n) for i, n in enumerate([16001, 733, 8000])]
    pcms = [odd[0], built("gc_pgru")[1], built("gc_len1")[1], built("gc_len0")[1], built("gc_len2")[1], odd[1], built("gc_len25")[1],
            built("gc_len47")[1], odd[2]]
    assert 3 * len(pcms) >= 17      # (chains of the launch: delay 3, a workgroup owns 16)
    batch = model.decode_batch(pcms)
    for i, p in enumerate(pcms):
        single = model.decode_batch([p])
        assert batch.num_frames(i) == single.num_frames(0)
        if single.num_frames(0) == 0:
            continue
        assert batch.words(i) == single.words(0) and batch.costs(i) == single.costs(0)
        for kind in (0, 2, 64):
            np.testing.assert_array_equal(batch.matrix(i, kind), single.matrix(0, kind))


def test_ragged_batch_of_an_output_gate_model(built):
    """The same for GrucKernel on gc_opgru's model: six utterances of three chains each, so a second workgroup with two chains."""
    from rhasspy_speech_amd import synth
    model, pcm = built("gc_opgru")
    pcms = [synth.synth_utterance(96 + i, n) for i, n in enumerate([16001, 733, 8000, 560, 4240])]
    pcms.insert(2, pcm)
    assert 3 * len(pcms) >= 17
    batch = model.decode_batch(pcms)
    for i, p in enumerate(pcms):
        single = model.decode_batch([p])
        assert batch.num_frames(i) == single.num_frames(0) > 0
        assert batch.words(i) == single.words(0) and batch.costs(i) == single.costs(0)
        for kind in (0, 2, 64):
            np.testing.assert_array_equal(batch.matrix(i, kind), single.matrix(0, kind))


def test_partial_and_endpoint_queries_leave_the_stream_unchanged(built):
    """A partial result and an endpoint query in mid-stream advance the stream like any advance: the recurrent state they leave is the
    one an advance leaves, and the finish result is bit for bit that of the undisturbed stream."""
    from rhasspy_speech_amd import _lib
    model, pcm = built("gc_stack")
    plain = _stream(model, pcm, 1024, True)
    st = _lib.Stream(model)
    for n, i in enumerate(range(0, len(pcm), 1024)):
        st.accept(pcm[i:i + 1024])
        if n == 9:
            st.partial()
        elif n == 17:
            st.endpoint()
        elif n % 3 == 0:
            st.advance()
    res = st.finish()
    for kind in (0, 1, 2):
        np.testing.assert_array_equal(res.matrix(0, kind), plain.matrix(0, kind))
    assert res.words(0) == plain.words(0) and res.costs(0) == plain.costs(0)


def test_a_clip_without_a_frame_fails_like_the_reference(built):
    """gc_len0: both reference binaries end with GetLattice's error; the result says the same."""
    from rhasspy_speech_amd import _lib
    g = lc.load_golden("gc_len0")
    assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
    model, pcm = built("gc_len0")
    res = model.decode_batch([pcm])
    assert res.num_frames(0) == 0
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        res.words(0)
    st = _lib.Stream(model)
    st.accept(pcm)
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        st.finish().words(0)
