"""Every layer GEMM instantiation the launch policy can plan, launched on the GPU at small shapes and held to the exact result.

tests/gemm_shape_cases.py has one row per (net, RS_GEMM_* switches, clip lengths); tests/test_gemm_shapes_cpu.py holds each row to the
real planner and the float64 oracle to a plain float64 evaluation.  Here, for every row, one batch call with keep_intermediates=1:
  1. the `gemm_launch:` lines of rs_model_describe are exactly the table's -- a case that drifts onto another kernel, grid or row
     count fails whatever its numbers say;
  2. every row of every utterance against oracle.pipeline.Nnet3.forward with float64 products on the device's own taps (features
     matrix(u, 0), iVector matrix(u, 1)): e_case <= 2 max(e_blas, e_exact) + 1e-7 max|loglike| and e_case < 1e-4, where e_blas is the
     FP32-BLAS oracle's error and e_exact the library's under RS_GEMM_B3=0 (the bound of
     test_split_fp16_gemm_is_as_close_to_exact_as_fp32_on_heavy_tailed_weights); a case that runs on the exact-FP32 kernels alone
     takes e_case <= 2 e_blas + 1e-7 max|loglike|;
  3. bit for bit: GemmKernelB3 / B3I / B3J tiles of any height, mixed or not, strip or not, make the same MFMAs in the same k order,
     so a split-family case equals the same clips on the baseline launch (RS_GEMM_B3J=0 RS_GEMM_B3I=0, RS_GEMM_CUS unset: everything
     on GemmKernelB3).  One documented rounding difference: a folded residual read from the operand image is the sum of two fp16 parts,
     within 2^-22 of the FP32 number (csrc/gemm_dev.h, res_img) -- the cases with such a residual are compared bit for bit with
     RS_GEMM_B3J=0 alone (GemmKernelB3I and its residual pass, which reads the same image) and held to (2) against the rest.  (This is
     the comparison that found GemmKernelB3J's in-register form fusing the residual's product and sum into one FMA: f256_f513,
     f256_f2049, f256_k32_f2049 and f256_k30_f2049 differed from the residual pass in 90 % of the log-likelihoods, by up to 3.1e-6.)
     The exact-family cases equal the RS_GEMM_B3=0 run without RS_GEMM_CUS, whatever tile height either chose;
  4. `range_retries=0 precision_retries=0 exact_fp32=0`: no silent repetition on the exact kernels;
  5. streams (STREAM_CASES): the advances of an incremental stream are the 32-row launches, and the finished stream's log-likelihoods
     equal, bit for bit, the same stream's on the other small-launch kernel (GemmKernelB3I<1, false, 8>; GemmKernelB3J's 32-row tiles
     for the case that asks for B3I) -- and the batch call's where the net has no iVector: a stream's iVector is estimated chunk by
     chunk, a batch call's over the whole utterance, so with an extractor the two calls do not compute the same thing.
The errors are a case's: the largest over every row of every utterance of its batch (printed per case); an utterance of 128 rows and
more is held to the bound with its own three errors as well.
Measured on one MI355X, e_case / e_blas / e_exact at max|loglike|: the largest e_case of a split-family case 5.72e-6 / 7.63e-6 / 9.30e-6
at 5.40 (f256_f2049), the case closest to its bound x270_f700 with 2.74e-6 / 2.09e-6 / 2.50e-6 at 2.75 (0.52 of the bound); exact family:
t250_f700_exact 3.58e-6 / 3.10e-6 / 3.58e-6 at 2.83 (0.55 of the bound).  79 tests, the whole file in 12.0 s; the slowest test 0.49 s."""
import contextlib
import os

import numpy as np
import pytest

from . import gemm_shape_cases as gsc

pytestmark = pytest.mark.gpu

LOGLIKE_TOL = 1e-4      # the project's (tests/test_gpu_parity.py)
BASELINE = {"RS_GEMM_B3J": "0", "RS_GEMM_B3I": "0"}
BASELINE_RES_IMG = {"RS_GEMM_B3J": "0"}      # image-read residuals: GemmKernelB3I and its residual pass
EXACT = {"RS_GEMM_B3": "0"}
SWITCHES = ("RS_GEMM_CUS", "RS_GEMM_B3", "RS_GEMM_B3I", "RS_GEMM_B3J", "RS_GEMM_B3J_WM", "RS_GEMM_B3J_MR", "RS_GEMM_B3J_SLOTS", "RS_GEMM_B3J_NARROW",
            "RS_GEMM_B3J_SMALL", "RS_GEMM_B3_NARROW", "RS_GEMM_B3_EXCLUSIVE", "RS_RESIDUAL_IMAGE")


@contextlib.contextmanager
def _switches(env):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """net -> (model_dir, graph_dir), written once."""
    from rhasspy_speech_amd import synth
    root = tmp_path_factory.mktemp("gemm_shapes")
    built = {}

    def get(net):
        if net not in built:
            spec = gsc.spec_of(net)
            synth.write_model_dir(root / net / "model", spec)
            synth.make_grammar_graph(root / net / "graph", spec)
            built[net] = (root / net / "model", root / net / "graph")
        return built[net]

    return get


def _clips(case):
    from rhasspy_speech_amd import synth
    return [synth.synth_utterance(700 + u, n) if n else np.zeros(0, np.int16) for u, n in enumerate(case["clips"])]


def _run(files, case, env):
    """One batch call of the case's clips on a model loaded under `env`: (gemm_launch lines, layer_gemm flags, per utterance the
    feature, iVector and log-likelihood matrices or None for an utterance without a frame)."""
    from rhasspy_speech_amd import _lib
    with _switches(env):
        model = _lib.Model(*files(case["net"]), _lib.default_opts(keep_intermediates=1, **case.get("opts", {})))
        res = model.decode_batch(_clips(case))
        text = model.describe().splitlines()
        utts = []
        for u, n in enumerate(case["clips"]):
            T = gsc.num_frames(n)
            fsf = case.get("opts", {}).get("frame_subsampling_factor", 1)
            assert res.num_frames(u) == (T + fsf - 1) // fsf
            iv = res.matrix(u, 1) if T and gsc.spec_of(case["net"]).ivector_dim else np.zeros((0, 0), np.float32)
            utts.append(None if T == 0 else (res.matrix(u, 0), iv, res.matrix(u, 2)))
        model.close()
    flags = [l for l in text if l.startswith("layer_gemm: ")]
    assert len(flags) == 1
    return [l for l in text if l.startswith("gemm_launch: ")], flags[0], utts


@pytest.fixture(scope="module")
def reference(files):
    """(net, clips, options) -> what the cases on those clips share: the baseline runs and the oracle's log-likelihoods (float64 and
    FP32-BLAS products) on the device's taps.  Computed once, not written to afterwards."""
    from oracle import pipeline
    done = {}

    def get(case):
        key = (case["net"], tuple(case["clips"]), tuple(sorted(case.get("opts", {}).items())))
        if key in done:
            return done[key]
        fsf = case.get("opts", {}).get("frame_subsampling_factor", 1)
        ref = {}
        runs = [("base", BASELINE), ("exact", EXACT)]
        if gsc.NETS[case["net"]].get("tdnnf"):
            runs += [("base_res_img", BASELINE_RES_IMG)]
        for name, env in runs:
            lines, flags, utts = _run(files, case, env)
            ref[name] = utts
            ref[name + "_flags"] = flags
        orc = pipeline.Oracle(*files(case["net"]))
        f64 = staticmethod(lambda x, wt: (x.astype(np.float64) @ wt.astype(np.float64)).astype(np.float32))
        blas = pipeline.Nnet3.matmul
        ref["f32"], ref["f64"] = [], []
        for u in ref["base"]:
            if u is None:
                ref["f32"].append(None); ref["f64"].append(None)
                continue
            feats, iv, _ = u
            rows = np.tile(iv[:1], (feats.shape[0] + 2 * orc.nnet.halo, 1)) if iv.size else None
            ref["f32"].append(orc.nnet.forward(feats, rows)[::fsf])
            try:
                pipeline.Nnet3.matmul = f64
                ref["f64"].append(orc.nnet.forward(feats, rows)[::fsf])
            finally:
                pipeline.Nnet3.matmul = staticmethod(blas)
        for v in ref.values():
            for a in (v if isinstance(v, list) else []):
                for m in (a if isinstance(a, tuple) else [a]):
                    if isinstance(m, np.ndarray):
                        m.setflags(write=False)
        done[key] = ref
        return ref

    return get


def _has_image_residual(case):
    return gsc.NETS[case["net"]].get("tdnnf", False) and case["env"].get("RS_RESIDUAL_IMAGE") != "0" and case["env"].get("RS_GEMM_B3I") != "0" and \
        case["env"].get("RS_GEMM_B3") != "0" and any(o["res"] for o in gsc.net_ops(gsc.spec_of(case["net"])))


@pytest.mark.parametrize("name", list(gsc.CASES))
def test_case_launches_what_the_table_says_and_is_exact(files, reference, name):
    case = gsc.CASES[name]
    lines, flags, utts = _run(files, case, case["env"])
    assert lines == gsc.expected_lines(case), "\n".join(lines)                                                    # 1
    exact_family = gsc.is_exact_case(case)
    if not exact_family:
        assert "range_retries=0 precision_retries=0 exact_fp32=0" in flags, flags                                # 4
    ref = reference(case)
    assert "range_retries=0 precision_retries=0 exact_fp32=0" in ref["base_flags"], ref["base_flags"]
    twin = ref["exact"] if exact_family else ref["base_res_img"] if _has_image_residual(case) else ref["base"]
    worst = [0.0, 0.0, 0.0, 0.0]
    for u, got in enumerate(utts):
        if got is None:
            continue
        # the taps do not depend on the layer GEMM's switches (the iVector branch's LDA runs on the exact kernels at whatever height)
        np.testing.assert_array_equal(got[0], ref["base"][u][0])
        np.testing.assert_array_equal(got[1], ref["base"][u][1])
        f64 = ref["f64"][u].astype(np.float64)
        scale = np.abs(f64).max()
        e_case = np.abs(got[2] - f64).max()
        e_blas = np.abs(ref["f32"][u] - f64).max()
        e_exact = np.abs(ref["exact"][u][2] - f64).max()
        assert got[2].shape == f64.shape
        worst = [max(a, b) for a, b in zip(worst, (e_case, e_blas, e_exact, scale))]
        np.testing.assert_array_equal(got[2], twin[u][2], err_msg=f"{name} utt {u}")                             # 3
        if got[2].shape[0] >= 128:      # (an utterance of a full tile and more is a sample large enough to carry the bound by itself)
            own = 2.0 * (e_blas if exact_family else max(e_blas, e_exact)) + 1e-7 * scale
            assert e_case <= own, (name, u, e_case, e_blas, e_exact, scale)
    # the errors of the CASE: the largest over every row of every utterance (a one-frame utterance's own 40 numbers are no yardstick)
    e_case, e_blas, e_exact, scale = worst
    print(f"{name} e_case={e_case:.3g} e_blas={e_blas:.3g} e_exact={e_exact:.3g} max|loglike|={scale:.3g}")
    bound = 2.0 * (e_blas if exact_family else max(e_blas, e_exact)) + 1e-7 * scale
    assert e_case <= bound, (name, e_case, e_blas, e_exact, scale)                                              # 2
    assert e_case < LOGLIKE_TOL, (name, e_case)


def test_nothing_is_recorded_without_keep_intermediates(files):
    from rhasspy_speech_amd import _lib, synth
    model = _lib.Model(*files("t250"), _lib.default_opts(keep_intermediates=0))
    model.decode_batch([synth.synth_utterance(700, 16000)])
    assert "layer_gemm: " in model.describe() and "gemm_launch:" not in model.describe()
    model.close()


def _stream(model, pcm):
    """The clip in 8192-byte pieces with a partial result after each (every tick's work, waited for); the labels of the image-fed
    launches the advances made; the finished stream's log-likelihoods."""
    from rhasspy_speech_amd import _lib
    st = _lib.Stream(model)
    raw = pcm.tobytes()
    seen = set()
    for k in range(0, len(raw), 8192):
        st.accept(raw[k:k + 8192])
        st.partial().close()
        for l in model.describe().splitlines():
            if l.startswith("gemm_launch: ") and l.endswith(" img=1") and " B3<" not in l:
                seen.add(gsc.label_of(l))
    res = st.finish(1, 1.0)
    ll = res.matrix(0, 2)
    res.close()
    st.close()
    return seen, ll


@pytest.mark.parametrize("name", list(gsc.STREAM_CASES))
def test_stream_advances_are_the_small_launches(files, name):
    from rhasspy_speech_amd import _lib, synth
    case = gsc.STREAM_CASES[name]
    pcm = synth.synth_utterance(900, case["samples"])
    out = {}
    # the twin runs the advances on the OTHER small-launch kernel: GemmKernelB3I<1, false, 8>, or (the case that asks for that one) GemmKernelB3J
    small_off = case["env"].get("RS_GEMM_B3J_SMALL") == "0"
    twin_env = {k: v for k, v in case["env"].items() if k != "RS_GEMM_B3J_SMALL"} if small_off else dict(case["env"], RS_GEMM_B3J_SMALL="0")
    for which, env in (("case", case["env"]), ("twin", twin_env)):
        with _switches(env):
            model = _lib.Model(*files(case["net"]), _lib.default_opts(keep_intermediates=1))
            out[which] = _stream(model, pcm)
            if which == "case":
                batch = model.decode_batch([pcm]).matrix(0, 2)
                assert "range_retries=0 precision_retries=0 exact_fp32=0" in model.describe()
            model.close()
    assert out["case"][0] == set(case["labels"]), out["case"][0]
    assert out["twin"][0] == ({"B3J<1,1,0,4,4,4>"} if small_off else {"B3I<1,0,8>"}), out["twin"][0]
    np.testing.assert_array_equal(out["case"][1], out["twin"][1])
    assert out["case"][1].shape == batch.shape
    if gsc.spec_of(case["net"]).ivector_dim == 0:
        np.testing.assert_array_equal(out["case"][1], batch)
