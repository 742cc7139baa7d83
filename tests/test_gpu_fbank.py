"""Log-mel filterbank models (--feature-type=fbank) on the GPU, through the C ABI, against what the reference's decoder binaries
gave for the cases of tests/fbank_cases.py (tests/golden/fbank/, written by tests/gen_fbank_golden.py).

Tolerances are test_gpu_parity.py's: words exact; filterbank rows with the log 2e-4 absolute (the power spectrum is the reference's
to the bit; what is left is the order of the mel sums and libm-vs-device logf); iVectors and log-likelihoods 1e-4; costs 2e-3
relative on the 1-best, rtol 2e-4 + atol 2e-3 on the 5-best.  Rows WITHOUT the log (fb40_linear, fb40_magnitude) are compared by
relative error: LINEAR_REL_TOL, see there."""
import numpy as np
import pytest

from tests import fbank_cases as fc

pytestmark = pytest.mark.gpu

FEAT_TOL = 2e-4
IVEC_TOL = 1e-4
LOGLIKE_TOL = 1e-4
# max |got - ref| / |ref| over the elements of the row matrix (every element is a sum of non-negative terms and none is zero: the
# dither is on).  Twice what the first GPU run measured against the goldens, 3.17e-7 for fb40_linear and 3.09e-7 for fb40_magnitude:
# a few float roundings of a filter's dot product, summed in another order than the reference's BLAS call.
LINEAR_REL_TOL = {"fb40_linear": 6.34e-7, "fb40_magnitude": 6.18e-7}
DECODED = [n for n in fc.CASES if n != "fb40_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model, pcm): the case's files written and its model loaded once (cases of one model_key share the model)."""
    from rhasspy_speech_amd import _lib
    models, done = {}, {}

    def get(name):
        if name not in done:
            key = fc.model_key(name)
            md, gd, _, pcm = fc.build_case_files(name, tmp_path_factory.mktemp(name))
            if key not in models:
                o = dict(keep_intermediates=1)
                o.update(fc.CASES[name].get("opts", {}))
                models[key] = _lib.Model(md, gd, _lib.default_opts(**o))
            done[name] = (models[key], pcm)
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
def test_offline_case(built, name):
    g = fc.load_golden(name)
    model, pcm = built(name)
    res = model.decode_batch([pcm], nbest=fc.NBEST)
    assert res.num_frames(0) == int(g["offline_num_frames"])
    feats = res.matrix(0, 0)
    assert feats.shape == g["input"].shape and feats.shape[1] == fc.expected_layout(name)[0]
    if name in fc.LINEAR:
        rel = float((np.abs(feats - g["input"]) / np.abs(g["input"])).max())
        print(f"{name}: rows up to {np.abs(g['input']).max():.4g}, max relative error {rel:.3g}")
        assert rel < LINEAR_REL_TOL[name], rel
    else:
        fd = float(np.abs(feats - g["input"]).max())
        print(f"{name}: rows up to {np.abs(g['input']).max():.4g}, max absolute error {fd:.3g}")
        assert fd < FEAT_TOL, fd
    if "offline_ivector" in g.files:
        assert np.abs(res.matrix(0, 1) - g["offline_ivector"]).max() < IVEC_TOL
    diff = float(np.abs(res.matrix(0, 2) - g["offline_loglikes"]).max())
    print(f"{name}: log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "offline")
    assert model.decode_batch([pcm], nbest=1).words(0) == res.words(0, 0)


def test_a_clip_without_a_frame_fails_like_the_reference(built):
    """fb40_len0: both reference binaries end with GetLattice's error; the result says the same."""
    from rhasspy_speech_amd import _lib
    g = fc.load_golden("fb40_len0")
    assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
    model, pcm = built("fb40_len0")
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
    return st.finish(nbest=fc.NBEST)


@pytest.mark.parametrize("mode", ["ticks", "one_block", "ragged"])
@pytest.mark.parametrize("name", DECODED)
def test_streamed_case(built, name, mode):
    """How the caller slices the audio and when it advances changes nothing: every pattern is held to the stream goldens."""
    g = fc.load_golden(name)
    model, pcm = built(name)
    res = _deliver(model, pcm, mode, len(name))
    assert res.num_frames(0) == int(g["stream_num_frames"])
    if "stream_ivector" in g.files:
        iv = res.matrix(0, 1)
        assert iv.shape == g["stream_ivector"].shape and np.abs(iv - g["stream_ivector"]).max() < IVEC_TOL
    assert np.abs(res.matrix(0, 2) - g["stream_loglikes"]).max() < LOGLIKE_TOL
    _check_nbest(res, g, "stream")


@pytest.mark.parametrize("name", ["fb40_iv", "fb80_noiv"])
def test_incremental_stream_equals_batch_replay(built, name, monkeypatch):
    """stream.cc against the batch replay of the same stream (RS_STREAM_BATCH=1): rows, iVectors, log-likelihoods bit for bit."""
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
        if kind == 1 and name == "fb80_noiv":
            continue
        np.testing.assert_array_equal(inc.matrix(0, kind), rep.matrix(0, kind))
    assert inc.words(0) == rep.words(0) and inc.costs(0) == rep.costs(0)


def test_ragged_batch_of_the_cases_that_share_a_model(built):
    """fb40_iv, fb40_len0 and fb40_len1 decode with one model: in one ragged batch (the clip without a frame in the middle, further
    clips of odd lengths around them) every utterance gets its single-utterance result bit for bit."""
    from rhasspy_speech_amd import synth
    names = [n for n in fc.CASES if fc.model_key(n) == fc.model_key("fb40_iv")]
    assert names == ["fb40_iv", "fb40_len0", "fb40_len1"]
    model = built("fb40_iv")[0]
    assert all(built(n)[0] is model for n in names)
    pcms = [built(n)[1] for n in names] + [synth.synth_utterance(60 + i, n) for i, n in enumerate([16001, 560, 24000])]
    batch = model.decode_batch(pcms)
    for i, p in enumerate(pcms):
        single = model.decode_batch([p])
        assert batch.num_frames(i) == single.num_frames(0)
        if single.num_frames(0) == 0:
            continue
        assert batch.words(i) == single.words(0) and batch.costs(i) == single.costs(0)
        for kind in (0, 1, 2):
            np.testing.assert_array_equal(batch.matrix(i, kind), single.matrix(0, kind))


def _rows(tmp_path, tag, bins, opts, pcm):
    """Filterbank rows of `pcm` from a model without extractor and without dither whose fbank.conf has `opts` on top of `bins` bins."""
    from rhasspy_speech_amd import _lib
    case = dict(spec=dict(feature_type="fbank", num_mel_bins=bins, fbank_opts=opts, ivector_dim=0, dither=0.0), graph="grammar", audio="zeros:0")
    md, gd, _, _ = fc.cases.build_case_files(case, tmp_path / tag)
    return _lib.Model(md, gd, _lib.default_opts(keep_intermediates=1)).decode_batch([pcm]).matrix(0, 0)


@pytest.mark.parametrize("bins", [40, 65])
def test_energy_column_shifts_the_mel_columns_and_nothing_else(tmp_path, bins):
    """The same spec apart from the flag, the same audio, no dither (whose seeds follow the network's set-up): with the energy in
    column 0 the mel columns are those of the model without it, one further right, bit for bit; with --htk-compat they stay and the
    energy follows them.  With 65 bins the shift carries bin 63 from the last lane of the first pass into column 64 and bin 64 --
    the second pass's only lane -- into column 65: a column dropped, doubled or clobbered at the 64-lane boundary shows here.  (A
    64-bin model is no reference for the first 64 columns of a 65-bin one: the triangles are spaced by the bin count.)"""
    from rhasspy_speech_amd import synth
    pcm = synth.synth_utterance(50, 16000)
    plain = _rows(tmp_path, "plain", bins, {}, pcm)
    first = _rows(tmp_path, "first", bins, {"use-energy": True}, pcm)
    last = _rows(tmp_path, "last", bins, {"use-energy": True, "htk-compat": True}, pcm)
    assert plain.shape == (98, bins) and first.shape == last.shape == (98, bins + 1)
    np.testing.assert_array_equal(first[:, 1:], plain)
    np.testing.assert_array_equal(last[:, :bins], plain)
    np.testing.assert_array_equal(first[:, 0], last[:, bins])
    # the raw log energy of a frame of this clip, computed here: log(sum((x - mean)^2)) over the 400 samples
    x = pcm[:400].astype(np.float64)
    assert abs(float(first[0, 0]) - np.log(((x - x.mean()) ** 2).sum())) < 1e-3
    assert len({tuple(r) for r in plain.T.tolist()}) == bins      # (no two columns alike)


@pytest.mark.parametrize("name", ["fb40_iv", "fb127_energy"])
def test_adaptation_round_trip(built, tmp_path, name):
    """The state taken from a finished stream opens the next one (also rebuilt from its arrays: same bits), and a state of an MFCC
    model whose rows are of another width is refused with the existing message.  fb127_energy: the widest row, 128 columns."""
    from rhasspy_speech_amd import _lib, synth
    model, pcm = built(name)

    def run(p, state):
        st = _lib.Stream(model, adaptation=state)
        for i in range(0, len(p), 4096):
            st.accept(p[i:i + 4096])
            st.advance()
        return st.finish(nbest=1), st.adaptation()

    r1, s1 = run(pcm, None)
    arr = s1.arrays()
    assert all(np.isfinite(v).all() for v in arr.values()) and any(v.size for v in arr.values())
    nxt = synth.synth_utterance(70, 20000)
    fresh, _ = run(nxt, None)
    carried, s2 = run(nxt, s1)
    again, _ = run(nxt, _lib.Adaptation.from_arrays(model, arr))
    np.testing.assert_array_equal(carried.matrix(0, 0), fresh.matrix(0, 0))            # the rows do not depend on the speaker
    assert np.abs(carried.matrix(0, 1) - fresh.matrix(0, 1)).max() > 1e-3              # the iVectors do
    for kind in (1, 2):
        np.testing.assert_array_equal(carried.matrix(0, kind), again.matrix(0, kind))
    assert carried.words(0) == again.words(0) and carried.costs(0) == again.costs(0)
    assert any(np.abs(s2.arrays()[k] - arr[k]).max() > 0 for k in arr if arr[k].size)
    # an MFCC model with the same extractor sizes but 20 cepstra
    other = dict(spec=dict(num_ceps=20), graph="grammar", audio="zeros:0")
    md, gd, _, _ = fc.cases.build_case_files(other, tmp_path / "mfcc20")
    m20 = _lib.Model(md, gd, _lib.default_opts(keep_intermediates=1))
    st = _lib.Stream(m20)
    st.accept(synth.synth_utterance(71, 16000))
    st.finish()
    with pytest.raises(_lib.RsError, match=r"the state's feature dimension \(20\) is not the model's"):
        _lib.Stream(model, adaptation=st.adaptation())


def test_describe_prints_the_fbank_line(built, tmp_path):
    from rhasspy_speech_amd import _lib, synth
    for name in fc.CASES:
        dim, bins, ecol = fc.expected_layout(name)
        s = fc.CASES[name]["spec"]
        o = s.get("fbank_opts", {})
        win = 1600 if s.get("frame_length") == 100.0 else 400
        line = (f"fbank: win={win} shift=160 padded={2048 if win == 1600 else 512} mel_bins={bins} dim={dim} use_energy={int(ecol >= 0)} "
                f"htk_compat={int(bool(o.get('htk-compat')))} use_log={int(o.get('use-log-fbank', True))} use_power={int(o.get('use-power', True))} "
                f"dither={s.get('dither', 1.0):g}\n")
        text = built(name)[0].describe()
        assert text.startswith(line), (name, text[:200])
    spec = synth.tiny_spec()
    synth.write_model_dir(tmp_path / "model", spec)
    synth.make_grammar_graph(tmp_path / "graph", spec)
    text = _lib.Model(tmp_path / "model", tmp_path / "graph").describe()
    assert text.startswith("mfcc: win=400 shift=160 padded=512 mel_bins=40 ceps=40 dither=1\nnnet_input_cmvn: 0\n") and "fbank" not in text
