"""TDNN-attention models (RestrictedAttentionComponent) without a GPU: the component reader, its checks and refusals, the set-up's
restatement (collapsed network, context, rand() position), the load-time planner through a stand-alone host program under the
address and undefined-behaviour sanitizers, the synthetic model writer, the goldens of tests/attention_cases.py and a float64
restatement of the case networks against them.  The tests that load a model fail on the commit before: the load was refused
("component type RestrictedAttentionComponent ... is not supported by the HIP acoustic-model kernels")."""
import ctypes as C
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import attention_cases as ac
from tests import cases

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in ac.CASES if n not in ac.NO_GOLDEN]
DECODED = [n for n in WITH_GOLDEN if n != "at_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = ac.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _mdl(model_dir):
    return model_dir / "model" / "model" / "final.mdl"


def test_goldens_are_there_for_every_case():
    for name in WITH_GOLDEN:
        g = ac.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(ac.CASES[name], sort_keys=True), name      # (made from this table)
        if name == "at_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "rand_calls", "collapsed", "chunk_l_r"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                                    for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "at_iv":
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        spec = cases.case_spec(ac.CASES[name])
        assert g["input"].shape[1] == spec.feat_dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape and int(g["offline_num_frames"]) <= 200
        assert int(g["offline_num_frames"]) == (g["input"].shape[0] + ac.fsf_of(name) - 1) // ac.fsf_of(name)
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
        # no near-ties: a build inside the log-likelihood bound cannot reorder the 5-best list
        for mode in ("offline", "stream"):
            total = g[f"{mode}_graph_cost"].astype(np.float64) + g[f"{mode}_acoustic_cost"]
            assert len(total) < 2 or np.diff(total).min() >= ac.MIN_NBEST_GAP, (name, mode, np.diff(total))
    frames = ac.plan(ac.CASES["at_basic"]["spec"]["attention_layers"][0])[0]
    assert [int(ac.load_golden(n)["offline_num_frames"]) for n in ("at_len1", "at_len2", "at_lenN")] == [1, 2, frames + 1]
    assert sorted(p.stem for p in ac.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in ac.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


FORM_OPS = {      # the ops of a layer behind its affine, by form: ReLU fuses into the affine, never into the attention op
    "attention-renorm-layer": ["gemm {n}.affine", "attention {n}.attention", "eltwise {n}.renorm"],
    "attention-relu-renorm-layer": ["gemm {n}.affine", "attention {n}.attention", "eltwise {n}.relu", "eltwise {n}.renorm"],
    "attention-relu-batchnorm-layer": ["gemm {n}.affine", "attention {n}.attention", "eltwise {n}.relu+{n}.batchnorm"],
    "relu-renorm-attention-layer": ["gemm {n}.affine+{n}.relu", "eltwise {n}.renorm", "attention {n}.attention"],
}


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_attention_ops(built, name):
    """One `op: attention` with one term and no fused stage and one `attention:` line per layer, the geometry the case's and the plan
    attention_cases.plan's (the planner's rule restated); the nodes around the component are the ops their form gives; the context
    is the reference's (golden chunk_l_r, and the offsets' sum through every layer)."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    ops = [l for l in text.splitlines() if l.startswith("op: ")]
    lines = [l for l in text.splitlines() if l.startswith("attention: ")]
    layers = ac.layers_of(name)
    assert len(lines) == len(layers) == sum(l.startswith("op: attention ") for l in ops) >= 1
    fsf = ac.fsf_of(name)
    for line, (k, layer) in zip(lines, layers):
        n = f"attention{k}"
        Cx, in_dim, out_dim = ac.synth.attention_layer_dims(layer)
        frames, hg, groups, rows, pitch, lds = ac.plan(layer)
        want = (f"attention: {n}.attention heads={layer['heads']} key={layer['key_dim']} value={layer['value_dim']} left={layer['left']} "
                f"right={layer['right']} stride={layer['stride']} key_scale={float(np.float32(ac.synth.attention_key_scale(layer))):.6g} "
                f"context={int(layer.get('output_context', True))} in={in_dim} out={out_dim} kernel=attn_valu<w8> frames={frames} heads_per_block={hg} "
                f"head_groups={groups} staged_rows={rows} pitch={pitch} lds={lds} grid=rows/{frames}x{groups}")
        assert line == want, (line, want)
        assert lds <= 64 * 1024
        form = FORM_OPS[layer.get("form", "attention-relu-renorm-layer")]
        first = next(i for i, l in enumerate(ops) if l.startswith("op: " + form[0].format(n=n) + " "))
        for i, f in enumerate(form):
            assert ops[first + i].startswith("op: " + f.format(n=n) + " out_dim="), (ops[first + i], f)
        op = next(l for l in ops if l.startswith(f"op: attention {n}.attention "))
        assert op.startswith(f"op: attention {n}.attention out_dim={out_dim} terms=1 stages=0"), op
        # under --frame-subsampling-factor the op runs on the rows its consumers read: every third one in both cases
        assert op.endswith(" rows=every-3") == (fsf == 3), op
    if name == "at_fsf3":      # stride 3: the op's source (its affine) is read at multiples of 3 only
        assert next(l for l in ops if l.startswith("op: gemm attention1.affine ")).endswith(" rows=every-3")
    if name == "at_fsf3_s2":   # stride 2: dense rows below the op
        assert "rows=every" not in next(l for l in ops if l.startswith("op: gemm attention1.affine "))
    if name == "at_recipe_head":
        assert ac.plan(layers[0][1])[2] > 1 and int(ac.load_golden(name)["offline_num_frames"]) > ac.plan(layers[0][1])[0]      # head groups, time tiles
    left, right = ac.contexts(name)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]
    if name != "at_len0":
        assert list(ac.load_golden(name)["chunk_l_r"]) == [24, left, right]


def test_mfcc_model_describes_itself_as_before(tmp_path):
    from rhasspy_speech_amd import _lib, synth
    spec = synth.tiny_spec()
    synth.write_model_dir(tmp_path / "model", spec)
    synth.make_grammar_graph(tmp_path / "graph", spec)
    text = _lib.Model(tmp_path / "model", tmp_path / "graph").describe()
    assert "attention" not in text
    assert [l.split()[1] for l in text.splitlines() if l.startswith("op: ")] == ["gemm"] * text.count("op: ")


@pytest.mark.parametrize("name", DECODED)
def test_setup_rand_position_and_collapsed_network(built, name):
    """rs_nnet3_setup (csrc/nnet3_setup.cc, host code): the number of rand() calls before the first frame is the one rs-dump measured
    on the reference -- the component's ReorderIndexes and PrecomputeIndexes draw nothing, so the position is certain and the
    reference's default dither works (at_dither_default) -- and the network CollapseModel leaves is the reference's, line for line
    (the FixedAffine folded into the first layer; nothing folds into or out of the attention component)."""
    from rhasspy_speech_amd import _lib
    lib = _lib.load_library()
    lib.rs_nnet3_setup_subsampled.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    md = built(name)[0]
    n, cert, buf = C.c_int64(), C.c_int32(), C.create_string_buffer(1 << 16)
    assert lib.rs_nnet3_setup_subsampled(str(_mdl(md)).encode(), 24, ac.fsf_of(name), C.byref(n), C.byref(cert), buf, len(buf)) == 0
    g = ac.load_golden(name)
    assert cert.value == 1
    assert n.value == int(g["rand_calls"]), (name, n.value)
    assert buf.value.decode().splitlines() == bytes(g["collapsed"]).decode().splitlines()
    assert any("component=attention1.attention input=" in l for l in buf.value.decode().splitlines())


def test_default_dither_model_loads(built):
    """at_dither_default: no --dither line, so the rows depend on the set-up's rand() position; the load accepts it (a network whose
    position is not certain is refused with a message)."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("at_dither_default")
    assert "dither=1" in _lib.Model(md, gd).describe().splitlines()[0]


def _refused(case, root, *needles):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = cases.build_case_files(case, root)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    for needle in needles:
        assert needle in str(ei.value), str(ei.value)


def test_required_inputs_that_are_a_subset_are_refused(built, tmp_path):
    """at_required_subset: the reference's set-up accepts the model (gen_attention_golden.py runs it); zero padding in time is
    refused here at load, with the node and the reason, and never decoded as something approximate.  The same to the right."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("at_required_subset")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert ac.REFUSAL in str(ei.value) and "(node attention1.attention)" in str(ei.value) and "not supported by the HIP acoustic-model kernels" in str(ei.value)
    right = dict(spec=ac._at((ac._a(right_required=0),)), graph="grammar", audio="zeros:0")
    _refused(right, tmp_path / "right", "(node attention1.attention)", "num-right-inputs-required 0 is smaller than num-right-inputs 1 (zero padding in time")


def test_sizes_beyond_the_kernel_plan_fail_the_load(tmp_path):
    _refused(dict(spec=ac._at((ac._a(key_dim=129),)), graph="grammar", audio="zeros:0"), tmp_path / "key",
             "attention attention1.attention: key-dim 129 is more than the 128 the HIP attention kernel takes")
    _refused(dict(spec=ac._at((ac._a(value_dim=130),)), graph="grammar", audio="zeros:0"), tmp_path / "value",
             "attention attention1.attention: value-dim 130 is more than the 128 the HIP attention kernel takes")
    _refused(dict(spec=ac._at((ac._a(left=20, right=12),)), graph="grammar", audio="zeros:0"), tmp_path / "context",
             "33 context positions (num-left-inputs + 1 + num-right-inputs); the HIP attention kernel takes at most 32")
    _refused(dict(spec=ac._at((ac._a(heads=65, key_dim=2, value_dim=2),)), graph="grammar", audio="zeros:0"), tmp_path / "heads",
             "65 heads; the HIP attention kernel takes at most 64")
    _refused(dict(spec=ac._at((ac._a(heads=1, key_dim=128, value_dim=128, left=16, right=15, stride=8),)), graph="grammar", audio="zeros:0"), tmp_path / "lds",
             "attention attention1.attention: the rows one frame reads (249 rows x (key-dim 128 + value-dim 128)", "do not fit the 65536 bytes of LDS")


def _edited_text_model(built, tmp_path, edits):
    md, gd, _, _ = built("at_text")
    dst = tmp_path / "model"
    shutil.copytree(md, dst)
    for f in (dst / "model" / "online" / "conf").iterdir():
        f.write_text(f.read_text().replace(str(md), str(dst)))
    text = _mdl(dst).read_text()
    for old, new in edits:
        assert text.count(old) >= 1, old
        text = text.replace(old, new, 1)
    _mdl(dst).write_text(text)
    return dst, gd


@pytest.mark.parametrize("old, new, needle", [
    ("<NumHeads> 2 ", "<NumHeads> 0 ", "Check() fails: num_heads_ > 0 && key_dim_ > 0 && value_dim_ > 0"),
    ("<NumLeftInputs> 2 <NumRightInputs> 1 ", "<NumLeftInputs> 0 <NumRightInputs> 0 ", "(num_left_inputs_ + num_right_inputs_) > 0"),
    ("<TimeStride> 1 ", "<TimeStride> 0 ", "Check() fails: time_stride_ > 0"),
    ("<NumLeftInputsRequired> 2 ", "<NumLeftInputsRequired> 3 ", "num_left_inputs_required_ <= num_left_inputs_"),
    ("<NumRightInputsRequired> 1 ", "<NumRightInputsRequired> -1 ", "num_right_inputs_required_ >= 0"),
    ("<KeyScale> 0.3535533845424652 ", "<KeyScale> 1.5 ", "Check() fails: key_scale_ > 0.0 && key_scale_ <= 1.0"),
    ("<StatsCount> 0.0 ", "<StatsCount> -1.0 ", "Check() fails: stats_count_ >= 0.0"),
    ("<ValueDim> 8 ", "<ValueDim> 9 ", "attention node attention1.attention expects input dim 58 but its descriptor provides 56"),
])
def test_what_the_reference_checks_is_checked(built, tmp_path, old, new, needle):
    """RestrictedAttentionComponent::Check()'s clauses and the input dimension, on at_text's model (text form) with one field of the
    component changed."""
    from rhasspy_speech_amd import _lib
    dst, gd = _edited_text_model(built, tmp_path, [(old, new)])
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    assert needle in str(ei.value) and "attention1.attention" in str(ei.value), str(ei.value)


_NODE = "component-node name=attention1.attention component=attention1.attention input="


@pytest.mark.parametrize("desc", ["Sum(attention1.affine, attention1.affine)", "Scale(0.5, attention1.affine)",
                                  "Append(attention1.affine, attention1.affine)"])
def test_a_sum_a_scale_or_an_append_feeding_the_component_is_refused(built, tmp_path, desc):
    from rhasspy_speech_amd import _lib
    dst, gd = _edited_text_model(built, tmp_path, [(_NODE + "attention1.affine", _NODE + desc)])
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    assert "attention node attention1.attention reads a Sum(), a Scale() or an Append() of several parts directly" in str(ei.value), str(ei.value)


def test_the_ivector_node_feeding_the_component_is_refused(built, tmp_path):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("at_iv")
    dst = tmp_path / "model"
    shutil.copytree(md, dst)
    for f in (dst / "model" / "online" / "conf").iterdir():
        f.write_text(f.read_text().replace(str(md), str(dst)))
    raw = _mdl(dst).read_bytes()
    old = (_NODE + "attention1.affine\n").encode()
    assert raw.count(old) == 1
    _mdl(dst).write_bytes(raw.replace(old, (_NODE + "ReplaceIndex(ivector, t, 0)\n").encode()))
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    assert "attention node attention1.attention reads the iVector input directly: not supported" in str(ei.value), str(ei.value)


def test_other_unknown_component_types_are_still_refused(built, tmp_path):
    """The catch-all of the op compiler, in its words, for a component type that is still not covered."""
    from rhasspy_speech_amd import _lib
    md = built("at_text")[0]
    text = _mdl(md).read_text()
    m = re.search(r"<ComponentName> attention1\.relu <RectifiedLinearComponent>.*?</RectifiedLinearComponent>", text, re.S)
    dst, gd = _edited_text_model(built, tmp_path, [(m.group(0), m.group(0).replace("RectifiedLinearComponent", "SoftmaxComponent"))])
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    assert "nnet3: component type SoftmaxComponent (node attention1.relu) is not supported by the HIP acoustic-model kernels" in str(ei.value)


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("at_basic")[:2]).describe()
    b = _lib.Model(*built("at_text")[:2]).describe()
    keep = ("op:", "attention:", "nnet:")
    assert [l for l in a.splitlines() if l.startswith(keep)] == [l for l in b.splitlines() if l.startswith(keep)]


def test_reader_and_planner_under_sanitizers(built, tmp_path):
    """tests/host/attention_plan_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's final.mdl,
    compiles the network, plans every attention op and walks the plan the way the kernel does; what the planner chose is held to
    tests/host/attention_plan_expected.txt."""
    from rhasspy_speech_amd import synth
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "attention_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "attention_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "attention_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args = []
    for name in ac.CASES:
        args += [name, str(_mdl(built(name)[0]))]
    extra = {
        "x_key_dim": dict(spec=ac._at((ac._a(key_dim=129),)), graph="grammar", audio="zeros:0"),
        "x_context": dict(spec=ac._at((ac._a(left=20, right=12),)), graph="grammar", audio="zeros:0"),
        "x_lds": dict(spec=ac._at((ac._a(heads=1, key_dim=128, value_dim=128, left=16, right=15, stride=8),)), graph="grammar", audio="zeros:0"),
        "x_recipe_size": dict(spec=ac._at((ac._a(heads=15, key_dim=40, value_dim=80, left=5, right=2, stride=3),)), graph="grammar", audio="zeros:0"),
        "x_widest": dict(spec=ac._at((ac._a(heads=64, key_dim=128, value_dim=128, left=1, right=0),)), graph="grammar", audio="zeros:0"),
    }
    for name, case in extra.items():
        mdl = tmp_path / name / "final.mdl"
        synth.write_final_mdl(mdl, cases.case_spec(case))
        args += [name, str(mdl)]
    p = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    expected = (ROOT / "tests" / "host" / "attention_plan_expected.txt").read_text()
    assert p.stdout == expected, p.stdout


# max |float64 restatement - golden offline_loglikes| per case, measured on the CPU when the goldens were made: the reference's FP32
# BLAS against exact arithmetic on its own input rows.  The test holds each to the project's 1e-4.
RESTATEMENT_MEASURED = {
    "at_basic": 1.328e-06, "at_form_renorm": 9.654e-07, "at_form_relu_renorm": 5.583e-07, "at_form_relu_batchnorm": 2.107e-06,
    "at_form_relu_renorm_attention": 8.591e-07, "at_odd": 6.052e-07, "at_left_only": 9.619e-07, "at_right_only": 7.883e-07,
    "at_stride3": 1.042e-06, "at_noctx": 8.584e-07, "at_keyscale": 1.231e-06, "at_sharp": 9.077e-06, "at_recipe_head": 1.622e-06,
    "at_stack": 1.860e-06, "at_fsf3": 8.358e-07, "at_fsf3_s2": 8.099e-07, "at_text": 1.328e-06, "at_len1": 5.148e-07,
    "at_len2": 5.972e-07, "at_lenN": 5.663e-07, "at_iv": 1.159e-06, "at_dither_default": 1.739e-06,
}


@pytest.mark.parametrize("name", DECODED)
def test_float64_restatement_agrees_with_the_reference(name):
    """attention_cases.Float64Net -- the row layouts of nnet-attention-component.h, key-scale, the context positions' rows, the
    softmax, output-context, NormalizeComponent -- from the golden `input` rows to log-likelihoods, against the reference's
    offline_loglikes.  Measured maxima (RESTATEMENT_MEASURED): the largest is at_sharp's, whose logits reach 146."""
    g = ac.load_golden(name)
    ll, taps, max_b = ac.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(taps) == len(ac.layers_of(name))
    for tap, (_, layer) in zip(taps, ac.layers_of(name)):
        assert tap.shape == (g["input"].shape[0], ac.synth.attention_layer_dims(layer)[2])
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}, max |b| {max_b:.4g}")
    assert diff < 1e-4, diff
    assert diff <= 2 * RESTATEMENT_MEASURED[name], diff
    if name == "at_sharp":
        assert max_b > 100.0


def test_the_writer_follows_the_reference_token_order():
    """RestrictedAttentionComponent::Write (nnet-attention-component.cc:442-471), text form: the tokens in its order, the required
    counts defaulting to the input counts, key-scale to 1 / sqrt(key-dim), empty statistics."""
    from rhasspy_speech_amd import synth
    w = synth.KaldiWriter(False)
    synth._w_attention(w, dict(heads=3, key_dim=4, value_dim=7, left=2, right=1, stride=3))
    text = w.getvalue().decode()
    assert re.findall(r"</?[A-Za-z]+>", text) == [
        "<RestrictedAttentionComponent>", "<NumHeads>", "<KeyDim>", "<ValueDim>", "<NumLeftInputs>", "<NumRightInputs>", "<TimeStride>",
        "<NumLeftInputsRequired>", "<NumRightInputsRequired>", "<OutputContext>", "<KeyScale>", "<StatsCount>", "<EntropyStats>", "<PosteriorStats>",
        "</RestrictedAttentionComponent>"]
    assert text.startswith("<RestrictedAttentionComponent> <NumHeads> 3 <KeyDim> 4 <ValueDim> 7 <NumLeftInputs> 2 <NumRightInputs> 1 <TimeStride> 3 "
                           "<NumLeftInputsRequired> 2 <NumRightInputsRequired> 1 <OutputContext> T <KeyScale> 0.5 <StatsCount> 0.0 <EntropyStats>")
    w = synth.KaldiWriter(False)
    synth._w_attention(w, dict(heads=1, key_dim=4, value_dim=7, left=2, right=1, stride=1, left_required=0, key_scale=0.25, output_context=False))
    assert "<NumLeftInputsRequired> 0 <NumRightInputsRequired> 1 <OutputContext> F <KeyScale> 0.25 " in w.getvalue().decode()
    assert synth.attention_layer_dims(dict(heads=3, key_dim=4, value_dim=7, left=2, right=1)) == (4, 3 * 19, 3 * 11)
    assert synth.attention_layer_dims(dict(heads=3, key_dim=4, value_dim=7, left=2, right=1, output_context=False)) == (4, 3 * 19, 3 * 7)


def test_node_and_component_names_are_the_xconfig_layers():
    """attention.py:139-249: <layer>.affine, then one component and node per word of the layer's name, each reading the one before."""
    from rhasspy_speech_amd import synth
    for form in synth.ATTENTION_FORMS:
        spec = synth.tiny_spec(**ac._at((ac._a(form=form),)))
        cfg, comps = synth.build_nnet(spec, np.random.default_rng(spec.seed))
        words = form.split("-")[:-1]
        names = ["attention1.affine"] + [f"attention1.{w}" for w in words]
        assert [n for n, _ in comps if n.startswith("attention1.")] == names
        lines = [l for l in cfg if " name=attention1." in l]
        assert lines == [f"component-node name={n} component={n} input={p}" for n, p in zip(names, ["tdnn2.batchnorm"] + names[:-1])]
        assert any(f"Offset({names[-1]}, -3)" in l for l in cfg if "name=tdnn3.affine" in l)
