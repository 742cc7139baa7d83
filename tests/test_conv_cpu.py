"""CNN-TDNN models (TimeHeightConvolutionComponent, PermuteComponent) without a GPU: the component reader, its checks and refusals,
the set-up's restatement (collapsed network, rand() position), the load-time planner through a stand-alone host program under the
address and undefined-behaviour sanitizers, the synthetic model writer, the goldens of tests/conv_cases.py and a float64 restatement
of the case networks against them."""
import ctypes as C
import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import cases
from tests import conv_cases as cc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in cc.CASES if n not in cc.NO_GOLDEN]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = cc.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _mdl(model_dir):
    return model_dir / "model" / "model" / "final.mdl"


def test_goldens_are_there_for_every_case():
    for name in WITH_GOLDEN:
        g = cc.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(cc.CASES[name], sort_keys=True), name      # (made from this table)
        if name == "cv_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "rand_calls"} | {f"{m}_{k}" for m in ("offline", "stream")
                                          for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "cv_recipe":
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        spec = cases.case_spec(cc.CASES[name])
        assert g["input"].shape[1] == spec.feat_dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape
        fsf = int(cc.CASES[name].get("conf_opts", {}).get("frame-subsampling-factor", 1))
        assert int(g["offline_num_frames"]) == (g["input"].shape[0] + fsf - 1) // fsf
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
    assert int(cc.load_golden("cv_len1")["offline_num_frames"]) == 1
    assert sorted(p.stem for p in cc.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in cc.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_convolutions(built, name):
    """The parent refused these directories at load ("component type TimeHeightConvolutionComponent ... is not supported").  Now
    they load on the host: one `op: conv` and one `conv:` line per convolution with the case's geometry, the ReLU and the block-dim
    BatchNorm fused into the op; cv_recipe's PermuteComponent over Append(idct-batchnorm, ivector-batchnorm) is a gather op."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    geo = cc.conv_geometry(name)
    ops = [l for l in text.splitlines() if l.startswith("op: conv ")]
    conv = [l for l in text.splitlines() if l.startswith("conv: ")]
    assert len(ops) == len(conv) == len(geo) >= 1
    fsf = int(cc.CASES[name].get("conf_opts", {}).get("frame-subsampling-factor", 1))
    for i, (fi, fo, hi, ho, sub, offs, toffs) in enumerate(geo, start=1):
        fused = f"cnn{i}.conv+cnn{i}.relu+cnn{i}.batchnorm"
        assert ops[i - 1].startswith(f"op: conv {fused} out_dim={ho * fo} terms={len(toffs)} stages=2"), ops[i - 1]
        head = (f"conv: {fused} filters={fi}->{fo} heights={hi}->{ho} sub={sub} offsets={len(offs)} time_offsets={len(toffs)} "
                f"k={len(offs) * fi} kernel=conv16x16x4<m")
        assert conv[i - 1].startswith(head), conv[i - 1]
        assert " rows_per_block=" in conv[i - 1] and " lds=" in conv[i - 1] and " grid=rows/" in conv[i - 1]
    if name == "cv_recipe":
        assert "op: gather combine-inputs out_dim=240 terms=2 stages=0\n" in text
        assert "op: gemm ivector-linear+ivector-batchnorm out_dim=200 k=10 segs=[-1:0:10] stages=1\n" in text
    else:
        assert "op: gather" not in text
    if fsf == 3:      # read through offsets that are multiples of 3 only: every third row, like the TDNN layers above them
        assert all(l.endswith(" rows=every-3") for l in ops), ops
    else:
        assert "rows=every" not in text
    # the context is the offsets' sum through every layer
    spec = cases.case_spec(cc.CASES[name])
    left = sum(-min(t) for *_, t in geo) + -min(spec.lda_offsets) + sum(-min(o) for o in spec.layer_offsets)
    right = sum(max(t) for *_, t in geo) + max(spec.lda_offsets) + sum(max(o) for o in spec.layer_offsets)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]


def test_mfcc_model_describes_itself_as_before(tmp_path):
    from rhasspy_speech_amd import _lib, synth
    spec = synth.tiny_spec()
    synth.write_model_dir(tmp_path / "model", spec)
    synth.make_grammar_graph(tmp_path / "graph", spec)
    text = _lib.Model(tmp_path / "model", tmp_path / "graph").describe()
    assert "conv" not in text and "gather" not in text
    assert [l.split()[1] for l in text.splitlines() if l.startswith("op: ")] == ["gemm"] * text.count("op: ")


@pytest.mark.parametrize("name", [n for n in WITH_GOLDEN])
def test_setup_rand_position_and_collapsed_network(built, name):
    """rs_nnet3_setup (csrc/nnet3_setup.cc, host code): the number of rand() calls before the first frame is the one rs-dump measured
    on the reference (every convolution step of the looped compilation draws in CheckModelAndIo, eight checks a step), and
    CollapseModel leaves these networks as they are written: a convolution is no affine component, the FixedAffine behind the stack
    reduces the dimension."""
    from rhasspy_speech_amd import _lib, synth
    lib = _lib.load_library()
    lib.rs_nnet3_setup_subsampled.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    md = built(name)[0]
    fsf = int(cc.CASES[name].get("conf_opts", {}).get("frame-subsampling-factor", 1))
    n, cert, buf = C.c_int64(), C.c_int32(), C.create_string_buffer(1 << 16)
    assert lib.rs_nnet3_setup_subsampled(str(_mdl(md)).encode(), 24, fsf, C.byref(n), C.byref(cert), buf, len(buf)) == 0
    assert cert.value == 1
    assert n.value == int(cc.load_golden(name)["rand_calls"]), (name, n.value)
    spec = cases.case_spec(cc.CASES[name])
    cfg, _ = synth.build_nnet(spec, np.random.default_rng(spec.seed))
    assert buf.value.decode().splitlines() == cfg


def _refused(case, root, needle):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = cases.build_case_files(case, root)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert needle in str(ei.value), str(ei.value)


def test_required_time_offsets_that_are_a_subset_are_refused(built):
    """cv_required_subset: the reference's set-up accepts the model (gen_conv_golden.py runs it); zero padding in time is refused
    here at load, in words that say so, and never decoded as something approximate."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("cv_required_subset")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert cc.REFUSAL in str(ei.value) and "cnn1.conv" in str(ei.value) and "zero padding in time" in str(ei.value)


def test_geometries_no_instantiation_covers_fail_the_load(tmp_path):
    nine = dict(spec=cc._fb((cc._l(8, 40, t=tuple(range(-4, 5))),)), graph="grammar", audio="zeros:0")
    _refused(nine, tmp_path / "nine", "9 distinct time offsets; the HIP convolution kernel takes at most 8")
    big = dict(spec=cc._fb((cc._l(300, 40), cc._l(8, 40))), graph="grammar", audio="zeros:0")
    _refused(big, tmp_path / "big", "do not fit the 98304 bytes of LDS")


@pytest.mark.parametrize("old, new, needle", [
    ("<HeightSubsampleOut> 1 ", "<HeightSubsampleOut> 0 ", "Convolution model fails basic check."),
    ("<RequiredTimeOffsets> [ -1 0 1 ]", "<RequiredTimeOffsets> [ -1 0 5 ]", "Required time offsets not a subset of all_time_offsets."),
    ("<NumFiltersIn> 1 ", "<NumFiltersIn> 2 ", "<LinearParams> is 8 x 9, the model needs 8 x 18"),
    ("<HeightOut> 40 ", "<HeightOut> 43 ", "no input is available"),
    ("<HeightIn> 40 <HeightOut> 40 ", "<HeightIn> 41 <HeightOut> 40 ", "expects input dim 41 but its descriptor provides 40"),
    ("[ -1,-1 -1,0 ", "[ -1,0 -1,-1 ", "offsets are not sorted and unique"),
])
def test_what_the_reference_checks_at_load_is_checked(built, tmp_path, old, new, needle):
    """ConvolutionModel::Check and the parameter dimensions, on cv_text's model (text form) with one field of its first convolution
    changed."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("cv_text")
    dst = tmp_path / "model"
    shutil.copytree(md, dst)
    for f in (dst / "model" / "online" / "conf").iterdir():
        f.write_text(f.read_text().replace(str(md), str(dst)))
    text = _mdl(dst).read_text()
    assert text.count(old) >= 1
    _mdl(dst).write_text(text.replace(old, new, 1))
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    assert needle in str(ei.value), str(ei.value)


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("cv_basic")[:2]).describe()
    b = _lib.Model(*built("cv_text")[:2]).describe()
    assert [l for l in a.splitlines() if l.startswith(("op:", "conv:", "nnet:"))] == [l for l in b.splitlines() if l.startswith(("op:", "conv:", "nnet:"))]


def test_reader_and_planner_under_sanitizers(built, tmp_path):
    """tests/host/conv_plan_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's final.mdl, compiles
    the network, plans every convolution and walks plan and weight image the way the kernel does; what the planner chose is held to
    tests/host/conv_plan_expected.txt."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "conv_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "conv_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "conv_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args = []
    for name in cc.CASES:
        args += [name, str(_mdl(built(name)[0]))]
    extra = {
        "x_nine_offsets": dict(spec=cc._fb((cc._l(8, 40, t=tuple(range(-4, 5))),)), graph="grammar", audio="zeros:0"),
        "x_lds": dict(spec=cc._fb((cc._l(300, 40), cc._l(8, 40))), graph="grammar", audio="zeros:0"),
        "x_recipe_size": dict(spec=cc._fb((cc._l(64, 40), cc._l(64, 40), cc._l(128, 20, sub=2), cc._l(256, 10, sub=2)), lda_offsets=(0,)),
                              graph="grammar", audio="zeros:0"),
        "x_tall": dict(spec=cc._fb((cc._l(4, 127),), bins=127, fbank_opts={"low-freq": 600, "high-freq": 0}), graph="grammar", audio="zeros:0"),
    }
    for name, case in extra.items():
        from rhasspy_speech_amd import synth
        mdl = tmp_path / name / "final.mdl"
        synth.write_final_mdl(mdl, cases.case_spec(case))
        args += [name, str(mdl)]
    p = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    expected = (ROOT / "tests" / "host" / "conv_plan_expected.txt").read_text()
    assert p.stdout == expected, p.stdout


# max |float64 restatement - golden offline_loglikes| per case, measured on the CPU when the goldens were made: the reference's FP32
# BLAS against exact arithmetic on its own input rows.  The test asserts twice that.
RESTATEMENT_MEASURED = {
    "cv_basic": 3.815e-07, "cv_recipe": 5.675e-07, "cv_nopad": 4.273e-07, "cv_odd": 3.432e-07, "cv_plus": 2.571e-07, "cv_t0": 5.829e-07,
    "cv_wide": 5.832e-07, "cv_m1": 2.635e-07, "cv_fsf3": 3.545e-07, "cv_text": 3.815e-07, "cv_len1": 1.634e-07,
}


@pytest.mark.parametrize("name", list(RESTATEMENT_MEASURED))
def test_float64_restatement_agrees_with_the_reference(name):
    """conv_cases.Float64Net -- the layouts of convolution.h:90-208, W's columns in (offset, filter) order, zero padding in height, the
    combine-feature-maps column map -- from the golden `input` rows to log-likelihoods, against the reference's offline_loglikes.
    Measured maxima (RESTATEMENT_MEASURED): 1.6e-07 (cv_len1, one frame) to 5.8e-07 (cv_wide); every case is far below the 5e-5 at
    which its weight scales would have had to change."""
    g = cc.load_golden(name)
    ll, layers = cc.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(layers) == len(cc.conv_geometry(name))
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}")
    assert RESTATEMENT_MEASURED[name] < 5e-5
    assert diff <= 2 * RESTATEMENT_MEASURED[name], diff


# sha256 over (relative path, bytes) of every file synth.write_model_dir(tiny_spec(**kw)) wrote on the commit before the
# convolutional fields were added to ModelSpec (the directory's own path replaced by <ROOT>)
PARENT_MODEL_SHA256 = {
    "tiny": (dict(), "09676d237fabef783f6ed1e813df44cbff9e1987a34446a24e54824537985ee5"),
    "tiny_text": (dict(binary=False), "e85b59f74ae8b5e856d4ebba742ebb1382d4535e70766baead3a978a0724bfc0"),
    "tiny_tdnnf_noiv": (dict(tdnnf=True, ivector_dim=0, seed=5), "004b2430aede82a792cdefb0565eb5ab434d3b9c3dad894ee07dfefd7665fb21"),
    "tiny_fbank_energy": (dict(feature_type="fbank", num_mel_bins=40, fbank_opts={"use-energy": True}),
                          "e57274fc943b1c4f1915dfae217af8ad1b847ee7d3e4a9e12837a17426d5862a"),
    "tiny_priors_softmax": (dict(with_priors=True, with_log_softmax=True, context="triphone"),
                            "aca5be905bdb0384f3a0ec033d85051a65f06277dc0d15cd7c0c660b776371bd"),
}


@pytest.mark.parametrize("key", list(PARENT_MODEL_SHA256))
def test_existing_specs_write_the_bytes_they_always_wrote(tmp_path, key):
    from rhasspy_speech_amd import synth
    kw, want = PARENT_MODEL_SHA256[key]
    synth.write_model_dir(tmp_path / "m", synth.tiny_spec(**kw))
    h = hashlib.sha256()
    for f in sorted((tmp_path / "m").rglob("*")):
        if f.is_file():
            h.update(str(f.relative_to(tmp_path / "m")).encode() + b"\0" + f.read_bytes().replace(str(tmp_path).encode(), b"<ROOT>"))
    assert h.hexdigest() == want


def test_writers_of_the_two_components(tmp_path):
    """Binary and text forms of <Offsets> (an integer pair vector) and <ColumnMap>, and combine-feature-maps' column order."""
    from rhasspy_speech_amd import synth
    wb, wt = synth.KaldiWriter(True), synth.KaldiWriter(False)
    for w in (wb, wt):
        w.int_pair_vector([(-1, 0), (0, 2)])
    assert wb.getvalue() == b"\0B\x04\x02\0\0\0" + np.array([-1, 0, 0, 2], "<i4").tobytes()
    assert wt.getvalue() == b"[ -1,0 0,2 ]\n"
    assert synth.combine_feature_maps(2, 1, 2) == [0, 2, 3, 1, 4, 5]
    assert synth.conv_layer_offsets(dict(time_offsets=(0, -1), height_offsets=(1, 0))) == [(-1, 0), (-1, 1), (0, 0), (0, 1)]
    assert synth.conv_layer_offsets(dict(offsets=((1, 0), (0, -1)))) == [(0, -1), (1, 0)]
