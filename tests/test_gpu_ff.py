"""Feed-forward nnet3 graph forms on the GPU, through the C ABI: the cases of tests/ff_cases.py against what the reference's decoder
binaries gave for them (tests/golden/ff/, written by tests/gen_ff_golden.py), against the float64 restatement of ff_cases.py on the
device's own features and iVector, and among themselves bit for bit.

Tolerances against the goldens are the other model families': words and 5-best exact; log-likelihoods 1e-4 absolute; costs 2e-3
relative on the 1-best, rtol 2e-4 + atol 2e-3 on the 5-best; iVectors 1e-4.  Against the restatement the bound is
tests/test_gpu_gemm_shapes.py's: e_case <= 2 e_blas + 1e-7 max|loglike| where every layer GEMM of the call ran on the exact-FP32
kernels, e_case <= 2 max(e_blas, e_exact) + 1e-7 max|loglike| where one ran on the split-fp16 family; e_blas is the FP32 CPU oracle's
error against float64 on the same taps, e_exact the library's under RS_GEMM_B3=0.  The three errors are printed per case.

Bit for bit: the 128-wide models on every split-fp16 kernel form the RS_GEMM_* switches reach (GemmKernelB3, B3I, B3J's 32-row tiles,
its 128-row tiles plain and in strip form) against the default launch; the three delivery patterns of a stream; every clip of a ragged batch against the clip alone; the rows of a
--frame-subsampling-factor=3 model against rows [::3] of the dense model on the same clip; RS_FUSE_RESIDUAL=0 against the default.

On the commit before, every test of the cases ff_cases.ROWWISE and their factor-3 twins failed with RunNnet's "row-wise component in
a fused position is not supported".

Measured on one MI355X, e_case / e_blas / e_exact at max|loglike|: the largest e_case 3.05e-6 / 3.10e-6 / 3.05e-6 at 7.19 (ff_segs16, exact
kernels); the largest of a case with split-fp16 launches 1.05e-6 / 7.54e-7 / 1.04e-6 at 7.14 (ff_range130); the case closest to its
bound ff_sums_fsf3 with 7.99e-7 / 5.01e-7 / 7.99e-7 at 1.56 (0.69 of the bound).  The whole file runs in a few seconds."""
import contextlib
import os

import numpy as np
import pytest

from tests import ff_cases as ff

pytestmark = pytest.mark.gpu

LOGLIKE_TOL = 1e-4
IVEC_TOL = 1e-4
DECODED = [n for n in ff.CASES if n not in ff.NO_FRAME + ff.NO_LOAD]
EXACT = (("RS_GEMM_B3", "0"),)
NO_FOLD = (("RS_FUSE_RESIDUAL", "0"),)
_ENV_KEYS = ("RS_GEMM_B3", "RS_GEMM_B3I", "RS_GEMM_B3J", "RS_GEMM_B3J_NARROW", "RS_GEMM_CUS", "RS_FUSE_RESIDUAL")


@contextlib.contextmanager
def _env(pairs):
    saved = {k: os.environ.pop(k, None) for k in _ENV_KEYS}
    os.environ.update(dict(pairs))
    try:
        yield
    finally:
        for k in _ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), written once per case."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = ff.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


@pytest.fixture(scope="module")
def offline(files):
    """(name, switches) -> (model, result of decode_batch([the case's clip], nbest 5), the kernels of that call's layer GEMM launches):
    each model loaded once per set of switches (cases of one model_key share it), each clip decoded once."""
    from rhasspy_speech_amd import _lib
    models, done = {}, {}

    def get(name, env=()):
        if (name, env) not in done:
            md, gd, _, pcm = files(name)
            with _env(env):
                mk = (ff.model_key(name), env)
                if mk not in models:
                    models[mk] = _lib.Model(md, gd, _lib.default_opts(keep_intermediates=1, stream_min_ticks=1))
                res = models[mk].decode_batch([pcm], nbest=ff.NBEST)
                done[(name, env)] = (models[mk], res, _labels(models[mk]))
        return done[(name, env)]
    return get


def _loglikes(res, u=0):
    m = res.matrix(u, 2)
    m.setflags(write=False)
    return m


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
def test_offline_case(offline, name):
    g = ff.load_golden(name)
    model, res, _ = offline(name)
    assert res.num_frames(0) == int(g["offline_num_frames"])
    assert np.abs(res.matrix(0, 1) - g["offline_ivector"]).max() < IVEC_TOL
    diff = float(np.abs(_loglikes(res) - g["offline_loglikes"]).max())
    print(f"{name}: log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "offline")


def _labels(model):
    """The kernel of every layer GEMM launch of the model's most recent call (the iVector branch's splice + LDA aside)."""
    from tests import gemm_shape_cases as gsc
    return [gsc.label_of(l) for l in model.describe().splitlines() if l.startswith("gemm_launch: ") and not gsc.op_of(l).startswith("ivector.")]


@pytest.mark.parametrize("name", DECODED)
def test_against_the_float64_restatement(files, offline, name):
    from oracle import pipeline
    model, res, labels = offline(name)
    feats, iv, got = res.matrix(0, 0), res.matrix(0, 1), _loglikes(res)
    f64 = ff.restate(name, feats=feats, ivector=iv[0])
    assert got.shape == f64.shape
    md, gd = files(name)[:2]
    orc = pipeline.Oracle(md, gd)
    rows = np.tile(iv[:1], (feats.shape[0] + 2 * orc.nnet.halo, 1))
    f32 = orc.nnet.forward(feats, rows)[::ff.fsf_of(name)]
    exact = _loglikes(offline(name, EXACT)[1])
    assert all(l.startswith("Exact<") for l in offline(name, EXACT)[2])
    scale = float(np.abs(f64).max())
    e_case, e_blas, e_exact = (float(np.abs(x - f64).max()) for x in (got, f32, exact))
    split = any(not l.startswith("Exact<") for l in labels)
    bound = 2.0 * (max(e_blas, e_exact) if split else e_blas) + 1e-7 * scale
    print(f"{name} e_case={e_case:.3g} e_blas={e_blas:.3g} e_exact={e_exact:.3g} max|loglike|={scale:.3g} of_bound={e_case / bound:.2f} "
          f"kernels={sorted(set(l.split('<')[0] for l in labels))}")
    assert e_case <= bound, (name, e_case, e_blas, e_exact, scale)
    assert e_case < LOGLIKE_TOL


@pytest.mark.parametrize("name", [n for n in DECODED if ff.CASES[n]["net"][0] == "chains"])
def test_stage_chains_on_the_exact_kernels(offline, name):
    """RS_GEMM_B3=0: the generic epilogue of the exact-FP32 family on the same chains, against the golden."""
    g = ff.load_golden(name)
    res = offline(name, EXACT)[1]
    diff = float(np.abs(_loglikes(res) - g["offline_loglikes"]).max())
    print(f"{name}: exact kernels, log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "offline")


# strip: GemmKernelB3J takes every image-fed launch of two rows and more (RS_GEMM_B3J=2), RS_GEMM_B3J_NARROW=0 keeps a 128-column layer
# off its 256 x 128 shape, which has no strip form: 128-row tiles, in strip form for a three-offset splice of one image
STEERED = {"b3i": (("RS_GEMM_B3J", "0"),), "b3": (("RS_GEMM_B3I", "0"), ("RS_GEMM_B3J", "0")), "cus8": (("RS_GEMM_CUS", "8"),),
           "strip": (("RS_GEMM_B3J", "2"), ("RS_GEMM_B3J_NARROW", "0"), ("RS_GEMM_CUS", "8"))}
SPLIT_CASES = ["ff_chains128_r0", "ff_chains128_r1", "ff_chains128_r2", "ff_chains128_r3", "ff_renorm128", "ff_range130"]


def _forms(labels):
    """{"Exact", "B3", "B3I", "B3J plain", "B3J strip"} of a call's launches (GemmKernelB3J<WM, MIXED, STRIP, ...>)."""
    out = set()
    for l in labels:
        fam = l.split("<")[0]
        out.add(fam if fam != "B3J" else "B3J strip" if l.split("<")[1].split(",")[2] == "1" else "B3J plain")
    return out


@pytest.mark.parametrize("steer", list(STEERED))
@pytest.mark.parametrize("name", SPLIT_CASES)
def test_every_split_kernel_gives_the_same_rows(offline, name, steer):
    """The 128-wide layers on GemmKernelB3I (RS_GEMM_B3J=0), on GemmKernelB3 alone (and RS_GEMM_B3I=0: no operand images, a
    NormalizeComponent's rows reach the next GEMM as floats), planned for 8 compute units, and on GemmKernelB3J's 128-row tiles -- strip
    form behind the (-1, 0, 1) and (-3, 0, 3) splices, plain behind a single segment: the tiles of the split-fp16 family make the same
    MFMAs in the same k order whatever their height and however their operands arrive, so the log-likelihoods are the default launch's
    bit for bit."""
    base, (model, res, labels) = offline(name), offline(name, STEERED[steer])
    forms = _forms(labels)
    print(f"{name} {steer}: {sorted(set(labels))}; default {sorted(set(base[2]))}")
    assert forms - {"Exact"}, forms
    if steer == "strip" and name != "ff_range130":      # (ff_range130's second layer reads four segments of two widths: no strip)
        assert "B3J strip" in forms, forms
        if "chains" in name:      # (the fourth layer reads one segment)
            assert "B3J plain" in forms, forms
    if steer == "b3i":
        assert "B3I" in forms and not any(f.startswith("B3J") for f in forms), forms
    if steer == "b3":
        assert forms == {"Exact", "B3"}, forms
    np.testing.assert_array_equal(_loglikes(res), _loglikes(base[1]))


@pytest.mark.parametrize("name", SPLIT_CASES[:4])
def test_the_stage_chains_ran_on_every_kernel_family(offline, name):
    """Each chain model over the steerings: GemmKernelB3 (float segments: the first layer), GemmKernelB3I, GemmKernelB3J in plain and in
    strip form, and the exact kernels (the 48-column output layer; all of ff_chains64_*).  The four rotations put every chain behind
    every layer, so every chain's epilogue runs in each of these kernels."""
    seen = set()
    for env in [()] + list(STEERED.values()):
        seen |= _forms(offline(name, env)[2])
    assert seen == {"Exact", "B3", "B3I", "B3J plain", "B3J strip"}, seen


def _stream(model, pcm, piece, advance, nbest=1):
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model)
    for i in range(0, len(pcm), piece):
        st.accept(pcm[i:i + piece])
        if advance:
            st.advance()
    return st.finish(nbest=nbest)


@pytest.mark.parametrize("name", DECODED)
def test_streamed_case(files, offline, name):
    """1024-sample ticks, advanced as they arrive (what online2-cli-nnet3-decode-faster reads at a time) against the stream golden;
    2048-sample pieces and everything-then-finish are bit for bit the same rows, words and costs."""
    g = ff.load_golden(name)
    model, pcm = offline(name)[0], files(name)[3]
    res = _stream(model, pcm, 1024, True, nbest=ff.NBEST)
    assert res.num_frames(0) == int(g["stream_num_frames"])
    iv = res.matrix(0, 1)
    assert iv.shape == g["stream_ivector"].shape and np.abs(iv - g["stream_ivector"]).max() < IVEC_TOL
    diff = float(np.abs(res.matrix(0, 2) - g["stream_loglikes"]).max())
    print(f"{name}: streamed log-likelihood max abs diff {diff:.3g}")
    assert diff < LOGLIKE_TOL, diff
    _check_nbest(res, g, "stream")
    for other in (_stream(model, pcm, 2048, True, nbest=ff.NBEST), _stream(model, pcm, len(pcm), False, nbest=ff.NBEST)):
        for kind in (0, 1, 2):
            np.testing.assert_array_equal(other.matrix(0, kind), res.matrix(0, kind))
        assert [other.words(0, k) for k in range(other.num_hyps(0))] == [res.words(0, k) for k in range(res.num_hyps(0))]
        assert [other.costs(0, k) for k in range(other.num_hyps(0))] == [res.costs(0, k) for k in range(res.num_hyps(0))]


RAGGED = list({ff.model_key(n): n for n in DECODED}.values())      # one case of every model of the family


@pytest.mark.parametrize("name", RAGGED)
def test_ragged_batch_equals_each_clip_alone(files, offline, name):
    """Every clip of the family that decodes with the case's model (the clips without a frame and of one frame among them), two of odd
    lengths and another case's clip in one batch: every utterance gets its single-utterance result bit for bit."""
    from rhasspy_speech_amd import synth
    model = offline(name)[0]
    own = [n for n in ff.CASES if ff.model_key(n) == ff.model_key(name)]
    if name == "ff_renorm128":
        assert own == ["ff_renorm128", "ff_renorm128_len0", "ff_renorm128_len1"]
    other = next(n for n in DECODED if n not in own)
    pcms = [synth.synth_utterance(190, 16001)] + [files(n)[3] for n in own] + [synth.synth_utterance(191, 733), files(other)[3]]
    batch = model.decode_batch(pcms)
    for i, p in enumerate(pcms):
        single = model.decode_batch([p])
        assert batch.num_frames(i) == single.num_frames(0)
        if single.num_frames(0) == 0:
            continue
        assert batch.words(i) == single.words(0) and batch.costs(i) == single.costs(0)
        for kind in (0, 1, 2):
            np.testing.assert_array_equal(batch.matrix(i, kind), single.matrix(0, kind))


@pytest.mark.parametrize("name", list(ff.DENSE_OF))
def test_factor_3_rows_are_the_dense_rows(files, offline, name):
    """The ops above the last layer with offsets that are no multiples of 3 run through strided row lists (ff_cases.net_ops: rows=every-3);
    what they compute for frame 3 i is what the dense model computes for it."""
    sub, dense = offline(name)[0], offline(ff.DENSE_OF[name])[0]
    assert ff.net_key(name) == ff.net_key(ff.DENSE_OF[name])
    assert any("rows=every-3" in l for l in sub.describe().splitlines() if l.startswith("op: "))
    pcm = files(name)[3]
    a, b = sub.decode_batch([pcm]), dense.decode_batch([pcm])
    assert a.num_frames(0) == (b.num_frames(0) + 2) // 3
    np.testing.assert_array_equal(a.matrix(0, 2), b.matrix(0, 2)[::3])


@pytest.mark.parametrize("name", ["ff_sums", "ff_sums_fsf3", "ff_rw_sum"])
def test_folded_residual_equals_the_elementwise_sum(offline, name):
    """RS_FUSE_RESIDUAL=0 keeps res.noop (tdnn1.renorm.sum) an elementwise op; the default folds it into the layer GEMM in front."""
    folded, plain = offline(name), offline(name, NO_FOLD)
    ops = lambda m: [l for l in m.describe().splitlines() if l.startswith("op: ")]
    assert len(ops(plain[0])) == len(ops(folded[0])) + 1 and any(" residual=" in l for l in ops(folded[0]))
    assert not any(" residual=" in l for l in ops(plain[0]))
    np.testing.assert_array_equal(_loglikes(folded[1]), _loglikes(plain[1]))
    assert folded[1].words(0) == plain[1].words(0) and folded[1].costs(0) == plain[1].costs(0)


def test_a_clip_without_a_frame_fails_like_the_reference(files, offline):
    from rhasspy_speech_amd import _lib
    g = ff.load_golden("ff_renorm128_len0")
    assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
    model, pcm = offline("ff_renorm128")[0], files("ff_renorm128_len0")[3]
    res = model.decode_batch([pcm])
    assert res.num_frames(0) == 0
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        res.words(0)
    st = _lib.Stream(model)
    st.accept(pcm)
    with pytest.raises(_lib.RsError, match="decoded no frames"):
        st.finish().words(0)
