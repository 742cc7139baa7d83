"""Models of sampling rates other than 16 kHz on the GPU, through the C ABI, against what the reference's decoder binaries gave for
the cases of tests/rate_cases.py (tests/golden/rates/, written by tests/gen_rate_golden.py): 8 kHz telephone models on the 256-point
transform, 22.05 and 32 kHz on the 1024-point one, 11.025 kHz on the 512-point and 44.1 / 48 kHz on the 2048-point one.

Tolerances are test_gpu_fbank.py's: words exact; rows 2e-4 absolute; iVectors and log-likelihoods 1e-4; costs 2e-3 relative on the
1-best, rtol 2e-4 + atol 2e-3 on the 5-best.  Offline everything is held to the reference.  Streamed, the words, costs and frame
count are held to the reference's stream binary (run with --samp-freq=<rate>); rs-dump cannot dump a stream at these rates, so the
streams' iVectors and log-likelihoods are held to oracle/pipeline.py's restatement of the stream, which tests/test_rates_cpu.py pins
to the same goldens."""
import numpy as np
import pytest

from tests import rate_cases as rc

pytestmark = pytest.mark.gpu

FEAT_TOL = 2e-4
IVEC_TOL = 1e-4
LOGLIKE_TOL = 1e-4
PAIR = ["r8k_iv", "r22k"]      # the 256- and the 1024-point transform


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model, pcm, model_dir, graph_dir): the case's files written and its model loaded once (cases of one model_key share
    the model)."""
    from rhasspy_speech_amd import _lib
    models, done = {}, {}

    def get(name):
        if name not in done:
            key = rc.model_key(name)
            md, gd, _, pcm = rc.build_case_files(name, tmp_path_factory.mktemp(name))
            if key not in models:
                models[key] = _lib.Model(md, gd, _lib.default_opts(keep_intermediates=1))
            done[name] = (models[key], pcm, md, gd)
        return done[name]
    return get


@pytest.fixture(scope="module")
def oracle_stream(built, tmp_path_factory):
    """name -> the oracle's transcript of the case's stream, computed once for the three delivery patterns."""
    done = {}

    def get(name):
        if name not in done:
            _, pcm, md, gd = built(name)
            done[name] = rc.make_oracle(name, md, gd, tmp_path_factory.mktemp(name + "_oracle")).transcribe_stream(pcm, nbest=rc.NBEST)
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


@pytest.mark.parametrize("name", rc.DECODED)
def test_offline_case(built, name):
    g = rc.load_golden(name)
    model, pcm = built(name)[:2]
    win, shift, padded = rc.geometry(name)
    assert f" win={win} shift={shift} padded={padded} " in model.describe().splitlines()[0]
    res = model.decode_batch([pcm], nbest=rc.NBEST)
    assert res.num_frames(0) == int(g["offline_num_frames"])
    feats = res.matrix(0, 0)
    assert feats.shape == g["input"].shape and feats.shape[1] == rc.feat_dim(name)
    fd = float(np.abs(feats - g["input"]).max())
    print(f"{name}: rows up to {np.abs(g['input']).max():.4g}, max absolute error {fd:.3g}")
    assert fd < FEAT_TOL, fd
    if "offline_ivector" in g.files:
        ivd = float(np.abs(res.matrix(0, 1) - g["offline_ivector"]).max())
        print(f"{name}: iVector max abs diff {ivd:.3g}")
        assert ivd < IVEC_TOL, ivd
    diff = float(np.abs(res.matrix(0, 2) - g["offline_loglikes"]).max())
    print(f"{name}: log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "offline")
    assert model.decode_batch([pcm], nbest=1).words(0) == res.words(0, 0)


def test_a_clip_without_a_frame_fails_like_the_reference(built):
    """r8k_len0, 199 samples: both reference binaries end with GetLattice's error; the result says the same."""
    from rhasspy_speech_amd import _lib
    g = rc.load_golden(rc.NO_FRAME)
    assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
    model, pcm = built(rc.NO_FRAME)[:2]
    res = model.decode_batch([pcm])
    assert res.num_frames(0) == 0
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        res.words(0)
    st = _lib.Stream(model)
    st.accept(pcm)
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        st.finish().words(0)


def _deliver(model, pcm, mode, seed):
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model)
    if mode == "ticks":                      # what online2-cli-nnet3-decode-faster reads at a time, advanced as it arrives
        for i in range(0, len(pcm), 1024):
            st.accept(pcm[i:i + 1024])
            st.advance()
    elif mode == "one_block":                # everything at the end
        st.accept(pcm)
    else:                                    # ragged pieces, an advance after every third
        rng = np.random.default_rng(seed)
        pos, k = 0, 0
        while pos < len(pcm):
            step = int(rng.integers(1, 9000))
            st.accept(pcm[pos:pos + step])
            pos += step
            k += 1
            if k % 3 == 0:
                st.advance()
    return st.finish(nbest=rc.NBEST)


@pytest.mark.parametrize("mode", ["ticks", "one_block", "ragged"])
@pytest.mark.parametrize("name", rc.DECODED)
def test_streamed_case(built, oracle_stream, name, mode):
    """How the caller slices the audio and when it advances changes nothing: every pattern gives the stream binary's words, costs and
    frame count, and the oracle's iVectors and log-likelihoods of that stream."""
    g = rc.load_golden(name)
    model, pcm = built(name)[:2]
    tr = oracle_stream(name)
    res = _deliver(model, pcm, mode, len(name))
    assert res.num_frames(0) == int(g["stream_num_frames"]) == tr.num_frames
    if tr.ivector is not None:
        iv = res.matrix(0, 1)
        assert iv.shape == tr.ivector.shape
        ivd = float(np.abs(iv - tr.ivector).max())
        print(f"{name}/{mode}: iVector max abs diff {ivd:.3g} over {iv.shape[0]} chunks")
        assert ivd < IVEC_TOL, ivd
    ll = res.matrix(0, 2)
    assert ll.shape == tr.loglikes.shape
    diff = float(np.abs(ll - tr.loglikes).max())
    print(f"{name}/{mode}: log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "stream")


@pytest.mark.parametrize("name", PAIR)
def test_incremental_stream_equals_batch_replay(built, name, monkeypatch):
    """stream.cc against the batch replay of the same stream (RS_STREAM_BATCH=1): rows, iVectors, log-likelihoods bit for bit."""
    from rhasspy_speech_amd import _lib
    model, pcm = built(name)[:2]

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
        np.testing.assert_array_equal(inc.matrix(0, kind), rep.matrix(0, kind))
    assert inc.words(0) == rep.words(0) and inc.costs(0) == rep.costs(0)


@pytest.mark.parametrize("name", PAIR)
def test_ragged_batch_of_the_cases_that_share_a_model(built, name):
    """One ragged batch -- for r8k_iv the three cases of its model, the clip without a frame in the middle; further clips of odd
    lengths around them, one a sample short of a second frame -- gives every utterance its single-utterance result bit for bit."""
    from rhasspy_speech_amd import synth
    names = [n for n in rc.CASES if rc.model_key(n) == rc.model_key(name)]
    assert names == (["r8k_iv", "r8k_len0", "r8k_len1"] if name == "r8k_iv" else ["r22k"])
    model = built(name)[0]
    assert all(built(n)[0] is model for n in names)
    win, shift, _ = rc.geometry(name)
    r = rc.rate(name)
    pcms = [built(n)[1] for n in names] + [synth.synth_utterance(60 + i, n, r) for i, n in enumerate([r + 1, win + shift - 1, r // 2 + 3, 0])]
    batch = model.decode_batch(pcms)
    for i, p in enumerate(pcms):
        single = model.decode_batch([p])
        assert batch.num_frames(i) == single.num_frames(0) == rc.num_frames(name, len(p))
        if single.num_frames(0) == 0:
            continue
        assert batch.words(i) == single.words(0) and batch.costs(i) == single.costs(0)
        for kind in (0, 1, 2):
            np.testing.assert_array_equal(batch.matrix(i, kind), single.matrix(0, kind))


@pytest.mark.parametrize("name", PAIR)
def test_the_model_says_its_rate_and_streams_check_theirs(built, name):
    """Model.sample_rate is the model's --sample-frequency; a stream transcriber left at the stream binary's default --samp-freq (16000)
    is refused with Kaldi's message before any audio is accepted, and one that names the model's rate decodes what a plain stream does."""
    import asyncio
    from rhasspy_speech_amd import _lib
    from rhasspy_speech_amd.transcribe_stream import KaldiNnet3StreamTranscriber
    model, pcm, md, gd = built(name)
    r = rc.rate(name)
    assert model.sample_rate == float(r)
    model.check_sample_rate(r)
    accepted = []

    async def audio():
        for i in range(0, len(pcm), 2048):
            accepted.append(i)
            yield pcm[i:i + 2048].tobytes()

    tr = KaldiNnet3StreamTranscriber(md, gd)
    with pytest.raises(RuntimeError, match=f"Sampling frequency mismatch, expected {r}, got 16000"):
        asyncio.run(tr.async_transcribe(audio(), gd))
    assert accepted == []
    with pytest.raises(_lib.RsError, match=f"Sampling frequency mismatch, expected {r}, got 16000"):
        model.check_sample_rate(16000)
    ok = KaldiNnet3StreamTranscriber(md, gd, samp_freq=r)
    st = ok._open_stream(ok._ensure_loaded())
    st.accept(pcm)
    assert st.finish(nbest=1).words(0) == parse_nbest(bytes(rc.load_golden(name)["stream_nbest_text"]))[0]


def test_stream_shim_decodes_with_samp_freq(built, tmp_path, monkeypatch):
    """online2-cli-nnet3-decode-faster --samp-freq=8000 (the shim, in this process) on the raw samples of r8k_iv: a lattice for "utt"."""
    import io
    import sys
    from rhasspy_speech_amd import kaldi_cli
    _, pcm, md, gd = built("r8k_iv")

    class _Stdin:
        buffer = io.BytesIO(pcm.astype("<i2").tobytes())
    monkeypatch.setattr(sys, "stdin", _Stdin)
    lat = tmp_path / "lat.ark"
    argv = ["--samp-freq=8000", f"--config={md / 'model' / 'online' / 'conf' / 'online.conf'}", "--max-active=7000", "--lattice-beam=8.0",
            "--acoustic-scale=1.0", "--beam=24.0", str(md / "model" / "model" / "final.mdl"), str(gd / "HCLG.fst"), str(gd / "words.txt"), f"ark:{lat}"]
    assert kaldi_cli.cli_main(argv) == 0
    assert lat.read_bytes().startswith(b"utt ") and lat.stat().st_size > 100
