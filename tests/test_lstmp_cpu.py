"""TDNN-LSTM models whose cell is spelled out as separate components (lstmp-layer / lstmp-batchnorm-layer / lstm-layer) without a
GPU: the goldens of tests/lstmp_cases.py, the float64 restatement against them, the recogniser of the composed block and its
refusals, the set-up's restatement on these networks (contexts, collapsed network, the dither rule), the reader's lowering and the
shared planner through a stand-alone host program under the address and undefined-behaviour sanitizers, and the synthetic model
writer.  On the commit before, every load below was refused: its parser stopped at the first peephole ("cannot determine the output
dimension of component 'lstm1.w_i.c' of type NaturalGradientPerElementScaleComponent"), and a cycle it could parse met "the cycle has no
LstmNonlinearityComponent; lstmp-layer ... not supported"."""
import ctypes as C
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import cases
from tests import lstm_cases as lc
from tests import lstmp_cases as lp

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in lp.CASES if n not in lp.NO_GOLDEN]
DECODED = [n for n in WITH_GOLDEN if n != "lp_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = lp.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _mdl(model_dir):
    return model_dir / "model" / "model" / "final.mdl"


# ------------------------------------------------------------------------------------------ goldens

def test_goldens_are_there_for_every_case():
    for name in WITH_GOLDEN:
        g = lp.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(lp.CASES[name], sort_keys=True), name      # (made from this table)
        if name == "lp_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "context", "collapsed"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                    for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "lp_stack":
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        spec = cases.case_spec(lp.CASES[name])
        assert g["input"].shape[1] == spec.feat_dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape
        fsf = lp.fsf_of(name)
        assert int(g["offline_num_frames"]) == (g["input"].shape[0] + fsf - 1) // fsf
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
    frames = {n: lp.load_golden(n)["input"].shape[0] for n in lp.LENGTHS[1:]}
    assert frames == {"lp_len1": 1, "lp_len2": 2, "lp_len25": 25, "lp_len47": 47}      # (the chunk is 24 frames)
    assert sorted(p.stem for p in lp.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in lp.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


@pytest.mark.parametrize("name", DECODED)
def test_nbest_hypotheses_are_far_enough_apart(name):
    """Adjacent n-best hypotheses differ in total cost by more than 0.02, ten times the 2e-3 cost tolerance of the GPU tests: the order
    of the list is not a matter of rounding."""
    g = lp.load_golden(name)
    for mode in ("offline", "stream"):
        total = g[f"{mode}_graph_cost"].astype(np.float64) + g[f"{mode}_acoustic_cost"]
        if len(total) > 1:
            assert np.diff(total).min() > 0.02, (name, mode, np.diff(total).min())


@pytest.mark.parametrize("name", DECODED)
def test_float64_restatement_agrees_with_the_reference(name):
    """lstmp_cases.Float64Net -- the composed recurrence over the golden `input` rows: the peepholes on the delayed cell, the cell
    scaled by its truncation component before the output gate's peephole and Tanh, the recurrent state by its own -- against the
    reference's offline_loglikes, within 2.5e-5: a quarter of the device bound, so that the reference's own FP32 rounding does not
    consume it.  Measured when the goldens were made: 1.9e-07 (lp_len2) to 1.3e-06 (lp_stack)."""
    g = lp.load_golden(name)
    ll, blocks = lp.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(blocks) == len(lp.block_dims(name))
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}")
    assert diff < 2.5e-5, diff
    if "offline_ivector" not in g.files:      # (without an extractor the streamed rows are the offline ones)
        np.testing.assert_array_equal(g["stream_loglikes"], g["offline_loglikes"])


def test_the_fast_block_s_order_is_another_function():
    """lp_decay's weights through LstmNonlinearityComponent's order (the truncation scale applied behind the output gate's peephole
    and Tanh, not before them) miss the reference's log-likelihoods by more than the device bound of 1e-4: a kernel that walked the
    composed block in the fast block's order would fail the case."""
    g = lp.load_golden("lp_decay")
    net = lp.Float64Net(cases.case_spec(lp.CASES["lp_decay"]), *lp.contexts("lp_decay"))
    net.fast_order = True
    diff = float(np.abs(net.forward(g["input"])[0] - g["offline_loglikes"]).max())
    print(f"lp_decay in the fast block's order: max |restatement - reference| {diff:.4g}")
    assert diff > 1e-4, diff


# ------------------------------------------------------------------------------------------ load and describe

def _block_lines(name):
    out = []
    for k, composed, in_dim, cell, rec, nonrec, delay, scale_c, scale_r, drop in lp.block_dims(name):
        rec_dim = rec if rec else cell
        lds = 16 * 4 * (2 * ((rec_dim + 15) // 16 * 16 + 4) + (((cell + 15) // 16 * 16 + 4) if rec else 0))
        if composed:
            out.append(f"lstmp: lstm{k}.c_t input={in_dim} cell={cell} rec={rec} nonrec={nonrec} delay={delay} scale_c={scale_c:g} scale_r={scale_r:g} "
                       f"dropout={drop} kernel=lstmp16x16x4<w8> rows_per_block=16 lds={lds} w_x={in_dim} w_r={rec_dim} cell_tiles={(cell + 15) // 16} "
                       f"out_tiles={(rec + nonrec + 15) // 16} grid=chains/16")
        else:
            out.append(f"lstm: lstm{k}.lstm_nonlin input={in_dim} cell={cell} rec={rec} nonrec={nonrec} delay={delay} scale={scale_c:g} dropout_mask={drop} "
                       f"kernel=lstm16x16x4<w8> rows_per_block=16 lds={lds} w_all={in_dim}+{rec_dim} cell_tiles={(cell + 15) // 16} "
                       f"out_tiles={(rec + nonrec + 15) // 16} grid=chains/16")
    return out


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_blocks(built, name):
    """The parent refused these directories at load (at the first peephole component; a cycle it could parse, with "the cycle has no
    LstmNonlinearityComponent; lstmp-layer ... not supported").  Now they load on the host: per composed block one layer GEMM over the four affines' stacked feed-forward columns, an `op: lstmp`
    and a `lstmp:` line with the case's dims, both scales and what the planner chose; the context is the reference's."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    dims = lp.block_dims(name)
    want = _block_lines(name)
    assert [l for l in text.splitlines() if l.startswith("lstmp: ")] == [l for l in want if l.startswith("lstmp: ")]
    assert [l for l in text.splitlines() if l.startswith("lstm: ")] == [l for l in want if l.startswith("lstm: ")]
    ops = [l for l in text.splitlines() if l.startswith("op: ")]
    walks = []
    for k, composed, in_dim, cell, *_r in dims:
        kind, node, gemm = ("lstmp", f"lstm{k}.c_t", f"lstm{k}.c_t.x") if composed else ("lstm", f"lstm{k}.lstm_nonlin", f"lstm{k}.W_all.x")
        at = [i for i, l in enumerate(ops) if l.startswith(f"op: {kind} {node} out_dim={2 * cell} terms=1 stages=0")]
        assert len(at) == 1 and ops[at[0] - 1].startswith(f"op: gemm {gemm} out_dim={4 * cell} k={in_dim} "), ops
        walks.append(at[0])
    assert walks == sorted(walks)      # (network order: what result matrix 64 + k counts)
    fsf = lp.fsf_of(name)
    block_ops = [l for l in ops if l.startswith("op: lstmp ")]
    if name == "lp_fsf3":        # delay 3 under factor 3 and offsets {-3, 0, 3} above: one residue class
        assert all(l.endswith(" rows=every-3") for l in block_ops)
    else:                        # (lp_fsf3_d2: delay 2 visits every class; the layers above it still run on every third row)
        assert not any("rows=every" in l for l in block_ops)
        assert ("rows=every-3" in text) == (fsf == 3)
    left, right = lp.contexts(name)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]
    if name != "lp_len0":
        assert [left, right] == lp.load_golden(name)["context"].tolist()      # (what the reference's looped decodable computed)
    if name == "lp_stack":       # BatchNorm on rp_t: an elementwise op of its own, the block's buffers stay as the block wrote them
        assert "op: eltwise lstm2.rp_t_batchnorm out_dim=24 terms=1 stages=1\n" in text
    if name == "lp_scales":
        assert " scale_c=0.9 scale_r=0.8 " in text
    if name == "lp_clipgrad":    # (a ClipGradientComponent has no scale)
        assert " scale_c=1 scale_r=1 " in text


def _setup(md, fsf):
    from rhasspy_speech_amd import _lib
    lib = _lib.load_library()
    lib.rs_nnet3_setup_subsampled.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    n, cert, buf = C.c_int64(), C.c_int32(), C.create_string_buffer(1 << 16)
    assert lib.rs_nnet3_setup_subsampled(str(_mdl(md)).encode(), 24, fsf, C.byref(n), C.byref(cert), buf, len(buf)) == 0
    return n.value, cert.value, buf.value.decode().splitlines()


@pytest.mark.parametrize("name", DECODED)
def test_setup_leaves_the_reference_s_network(built, name):
    """rs_nnet3_setup (csrc/nnet3_setup.cc, host code) on these networks: the collapsed network is the one rs-dump printed after the
    reference's CollapseModel (the lda transform folded into the first TDNN layer; of a block nothing collapses -- its affines are read
    through Append(), its dropout stands behind a sigmoid: its lines are those synth.py wrote); the rand() position is reported as
    not certain."""
    from rhasspy_speech_amd import synth
    _, certain, lines = _setup(built(name)[0], lp.fsf_of(name))
    assert certain == 0
    assert lines == bytes(lp.load_golden(name)["collapsed"]).decode().splitlines()
    spec = cases.case_spec(lp.CASES[name])
    written = [l for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if " name=lstm" in l]
    assert len(written) >= 17 and [l for l in lines if " name=lstm" in l] == written


def test_default_dither_is_refused_with_the_recurrence_named(built):
    """lp_dither_default: the reference's set-up accepts the model (gen_lstmp_golden.py runs it); the rand() calls of a recurrent
    compilation are not replayed, so by the existing rule the model loads with --dither=0 only."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("lp_dither_default")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    msg = str(ei.value)
    assert "--dither=1" in msg and "cannot be derived for this network" in msg and "the network is recurrent (a cycle through node lstm1." in msg, msg


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("lp_basic")[:2]).describe()
    b = _lib.Model(*built("lp_text")[:2]).describe()
    keep = ("op:", "lstmp:", "nnet:")
    assert [l for l in a.splitlines() if l.startswith(keep)] == [l for l in b.splitlines() if l.startswith(keep)]
    assert any(l.startswith("lstmp:") for l in a.splitlines())


# ------------------------------------------------------------------------------------------ refusals

def _edited(src, tmp_path, edit):
    """A text-form model directory with its final.mdl passed through `edit`."""
    md, gd = src[:2]
    dst = tmp_path / "model"
    shutil.copytree(md, dst)
    for f in (dst / "model" / "online" / "conf").iterdir():
        f.write_text(f.read_text().replace(str(md), str(dst)))
    text = _mdl(dst).read_text()
    new = edit(text)
    assert new != text
    _mdl(dst).write_text(new)
    return dst, gd


def _swap(old, new, count=1):
    def edit(text):
        assert text.count(old) == count, (old, text.count(old))
        return text.replace(old, new)
    return edit


def _in_line(node, old, new):
    """Replaces `old` by `new` in the config line of `node` only."""
    def edit(text):
        lines = text.split("\n")
        at = [i for i, l in enumerate(lines) if l.startswith(f"component-node name={node} ")]
        assert len(at) == 1 and lines[at[0]].count(old) == 1, (node, old)
        lines[at[0]] = lines[at[0]].replace(old, new)
        return "\n".join(lines)
    return edit


def _other_input(text):
    """f1_t over another feed-forward input than the other three affines: Offset(x, -1)."""
    m = re.search(r"component-node name=lstm1\.f1_t component=lstm1\.W_f\.xr input=Append\(([^,]+), ", text)
    return _in_line("lstm1.f1_t", f"Append({m.group(1)}, ", f"Append(Offset({m.group(1)}, -1), ")(text)


_R3, _C3 = "IfDefined(Offset(lstm1.r_t, -3))", "IfDefined(Offset(lstm1.c_t, -3))"

REFUSED = {
    "the auxiliary c_t read from outside": (_swap("component=prefinal-chain.affine input=tdnn3.batchnorm", "component=prefinal-chain.affine input=Sum(tdnn3.batchnorm, lstm1.c_t)"),
                                            ["cycle at node lstm1.c_t", "the node is read from outside the block, by prefinal-chain.affine"]),
    "gates over different inputs": (_other_input, ["cycle at node lstm1.f1_t", "the four gates do not read the same feed-forward input"]),
    "two delays": (_in_line("lstm1.f1_t", _R3, "IfDefined(Offset(lstm1.r_t, -2))"), ["cycle at node lstm1.f1_t", "two different delays in one block, 2 and 3"]),
    "a positive delay": (_in_line("lstm1.f1_t", _R3, "IfDefined(Offset(lstm1.r_t, 3))"), ["cycle at node lstm1.f1_t", "a positive delay, Offset(lstm1.r_t, 3)"]),
    "a delay of 9": (lambda t: _swap(_R3, "IfDefined(Offset(lstm1.r_t, -9))", 4)(_swap(_C3, "IfDefined(Offset(lstm1.c_t, -9))", 3)(t)),
                     ["cycle at node lstm1.c1_t", "a delay of 9 frames; the HIP kernel takes 1 to 8"]),
    "the output peephole on the delayed cell": (_in_line("lstm1.o2_t", "input=lstm1.c_t", "input=" + _C3),
                                                ["cycle at node lstm1.o2_t", "the output gate's peephole does not read the current cell lstm1.c_t"]),
    "an input peephole on the current cell": (_in_line("lstm1.i2_t", "input=" + _C3, "input=lstm1.c_t"),
                                              ["cycle at node lstm1.i2_t", "the peephole reads lstm1.c_t of the current row, not IfDefined(Offset(lstm1.c_t, -delay))"]),
    "a peephole on the recurrent state": (_in_line("lstm1.f2_t", "input=" + _C3, "input=IfDefined(Offset(lstm1.r_t_preclip, -3))"),
                                          ["cycle at node lstm1.f2_t", "the peephole reads lstm1.r_t_preclip, not lstm1.c_t"]),
    "the state not through IfDefined": (_in_line("lstm1.g1_t", _R3, "Offset(lstm1.r_t, -3)"), ["cycle at node lstm1.g1_t", "is not inside IfDefined()"]),
    "weights of the wrong shape": (_in_line("lstm1.g1_t", "component=lstm1.W_c.xr", "component=lstm1.W_rp.m"),
                                   ["cycle at node lstm1.g1_t", "the affine has 16 rows, not the cell's dim 32"]),
    "h_t over another node": (_in_line("lstm1.h_t", "input=lstm1.c_t", "input=lstm1.c1_t"), ["cycle at node lstm1.h_t", "h_t is not a TanhComponent node over the cell lstm1.c_t"]),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_cycles_that_are_no_composed_block_are_refused(built, tmp_path, what):
    """Anything cyclic that is not exactly what lstmp-layer / lstm-layer emit stays refused at load, with the node and the reason:
    lp_text's config text with one thing changed."""
    from rhasspy_speech_amd import _lib
    edit, needles = REFUSED[what]
    dst, gd = _edited(built("lp_text"), tmp_path, edit)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    msg = str(ei.value)
    assert "recurrent networks are supported only as fast-lstmp-layer / fast-lstm-layer blocks" in msg, msg
    for needle in needles:
        assert needle in msg, (needle, msg)


def _refused(case, root, needle):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = cases.build_case_files(case, root)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert needle in str(ei.value), str(ei.value)


def test_sizes_beyond_the_plan_s_limits_fail_the_load(tmp_path):
    big = dict(spec=lp._lp((lp._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(big, tmp_path / "cell", "recurrent block lstm1.c_t: cell dim 2304 is more than the 2048 the HIP kernel takes")
    lds = dict(spec=lp._lp((lp._b(cell=1200, rec=0, nonrec=0),)), graph="grammar", audio="zeros:0")
    _refused(lds, tmp_path / "lds", "do not fit the 147456 bytes of LDS the HIP kernel keeps them in")


def _add_components(text, comps, nodes, rewire):
    """Appends text-form components and config lines to a text model and applies the (old, new) replacements of `rewire`."""
    from rhasspy_speech_amd import synth
    for old, new in rewire:
        text = _swap(old, new)(text)
    head, rest = text.split("\n\n<NumComponents> ", 1)
    count, rest = rest.split(" ", 1)
    body, tail = rest.rsplit("</Nnet3>", 1)
    for name, fn in comps:
        w = synth.KaldiWriter(False)
        w.token("<ComponentName>").token(name)
        fn(w)
        body += w.getvalue().decode() + "\n"
    return head + "\n" + "\n".join(nodes) + "\n\n<NumComponents> " + str(int(count) + len(comps)) + " " + body + "</Nnet3>" + tail


def _lstmb_shaped(text):
    """A node between W_all and the nonlinearity, as lstmb-layer's W_all_b / W_all_b_so stand there (ls_text's fast block edited)."""
    from rhasspy_speech_amd import synth
    return _add_components(text, [("lstm1.W_all_b_so", lambda w: synth._w_noop(w, 128))],
                           ["component-node name=lstm1.W_all_b_so component=lstm1.W_all_b_so input=lstm1.W_all"],
                           [("input=Append(lstm1.W_all, IfDefined(Offset(lstm1.c_trunc, -3)))", "input=Append(lstm1.W_all_b_so, IfDefined(Offset(lstm1.c_trunc, -3)))")])


def _non_fast_gru(text):
    """A cell in the manner of the non-fast gru-layer (xconfig/gru.py: XconfigGruLayer): sigmoid and tanh gates, two
    ElementwiseProductComponents, their Sum() through one BackpropTruncationComponent -- no second truncation node, no peepholes."""
    from rhasspy_speech_amd import synth
    rng = np.random.default_rng(4)
    W = (rng.standard_normal((32, 64)) / 8).astype(np.float32)
    comps = [("gz.W", lambda w: synth._w_affine(w, "NaturalGradientAffineComponent", W, np.zeros(32, np.float32))),
             ("gz.sig", lambda w: synth._w_nonlinear(w, "SigmoidComponent", 32)),
             ("gz.tanh", lambda w: synth._w_nonlinear(w, "TanhComponent", 32)),
             ("gz.y1", lambda w: synth._w_elementwise_product(w, 64, 32)),
             ("gz.y2", lambda w: synth._w_elementwise_product(w, 64, 32)),
             ("gz.s", lambda w: synth._w_backprop_truncation(w, 32, 1.0, 3))]
    nodes = ["component-node name=gz.W component=gz.W input=Append(tdnn3.batchnorm, IfDefined(Offset(gz.s_t, -3)))",
             "component-node name=gz.z_t component=gz.sig input=gz.W",
             "component-node name=gz.h_t component=gz.tanh input=gz.W",
             "component-node name=gz.y1_t component=gz.y1 input=Append(gz.z_t, IfDefined(Offset(gz.s_t, -3)))",
             "component-node name=gz.y2_t component=gz.y2 input=Append(gz.z_t, gz.h_t)",
             "component-node name=gz.s_t component=gz.s input=Sum(gz.y1_t, gz.y2_t)"]
    rewire = [("component=prefinal-chain.affine input=tdnn3.batchnorm", "component=prefinal-chain.affine input=gz.s_t")]
    return _add_components(text, comps, nodes, rewire)


STILL_REFUSED = {
    "an lstmb-layer-shaped cycle": (_lstmb_shaped, ["cycle at node lstm1.W_all_b_so", "the nonlinearity's first input is not an affine component node of the cycle"]),
    "a non-fast GRU cycle": (_non_fast_gru, ["cycle at node gz.s_t", "the cycle has no LstmNonlinearityComponent", "lstmp-layer", "the non-fast GRU layers are not supported",
                                            "it has no recurrent state node r_t"]),
}


@pytest.mark.parametrize("what", list(STILL_REFUSED))
def test_other_recurrent_layers_are_still_refused(tmp_path, what):
    from rhasspy_speech_amd import _lib
    edit, needles = STILL_REFUSED[what]
    src = lc.build_case_files("ls_text", tmp_path / "src")
    dst, gd = _edited(src, tmp_path, edit)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    msg = str(ei.value)
    assert "recurrent networks are supported only as fast-lstmp-layer / fast-lstm-layer blocks" in msg, msg
    for needle in needles:
        assert needle in msg, (needle, msg)


# ------------------------------------------------------------------------------------------ reader and planner under sanitizers

def test_reader_and_planner_under_sanitizers(built, tmp_path):
    """tests/host/lstmp_plan_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's final.mdl, runs the
    recogniser and the lowering, plans every block and compares the weight images element by element; what it prints is what
    describe() says.  The refused edits go through it as well: the recogniser's refusal paths run under the sanitizers too."""
    from rhasspy_speech_amd import _lib, synth
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "lstmp_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "lstmp_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "lstm_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args, want = [], []
    for name in lp.CASES:
        args += [name, str(_mdl(built(name)[0]))]
        if name in lp.NO_GOLDEN:      # (the dither rule is the engine's, not the reader's: the network itself plans like lp_basic's)
            want += [f"{name} {l}" for l in _block_lines(name)]
        else:
            text = _lib.Model(*built(name)[:2]).describe()
            want += [f"{name} {l}" for l in text.splitlines() if l.startswith(("lstmp: ", "lstm: "))]
    extra = {
        "x_full_size": (dict(spec=lp._lp((lp._b(cell=1024, rec=256, nonrec=256),)), graph="grammar", audio="zeros:0"),
                        "x_full_size lstmp: lstm1.c_t input=32 cell=1024 rec=256 nonrec=256 delay=3 scale_c=1 scale_r=1 dropout=0 kernel=lstmp16x16x4<w8> "
                        "rows_per_block=16 lds=99072 w_x=32 w_r=256 cell_tiles=64 out_tiles=32 grid=chains/16"),
        "x_cell": (dict(spec=lp._lp((lp._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0"),
                   "x_cell error: nnet3: recurrent block lstm1.c_t: cell dim 2304 is more than the 2048 the HIP kernel takes"),
        "x_plain": (dict(spec=dict(), graph="grammar", audio="zeros:0"), "x_plain no recurrent block"),
    }
    for name, (case, line) in extra.items():
        mdl = tmp_path / name / "final.mdl"
        synth.write_final_mdl(mdl, cases.case_spec(case))
        args += [name, str(mdl)]
        want.append(line)
    for i, (what, (edit, needles)) in enumerate(REFUSED.items()):
        dst, _ = _edited(built("lp_text"), tmp_path / f"refused{i}", edit)
        args += [f"r{i}", str(_mdl(dst))]
        want.append((f"r{i} error: ", needles))
    p = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    got = p.stdout.splitlines()
    assert len(got) == len(want), p.stdout
    for g, w in zip(got, want):
        if isinstance(w, tuple):
            assert g.startswith(w[0]) and all(n in g for n in w[1]), (g, w)
        else:
            assert g == w, (g, w)


# ------------------------------------------------------------------------------------------ the synthetic model writer

def test_specs_without_the_key_write_the_fast_block(tmp_path):
    """form defaults to the fast block: the same bytes with and without form="fast" (the digests of the parent's bytes are pinned by
    the test_existing_specs_write_the_bytes_they_always_wrote tests of the lstm / gru / pgru suites, and the goldens of
    tests/golden/lstm are compared with the models written today)."""
    from rhasspy_speech_amd import synth
    a, b = tmp_path / "a.mdl", tmp_path / "b.mdl"
    synth.write_final_mdl(a, cases.case_spec(lc.CASES["ls_stack"]))
    layers = tuple(dict(l, form="fast") for l in lc.CASES["ls_stack"]["spec"]["lstm_layers"])
    synth.write_final_mdl(b, cases.case_spec(dict(lc.CASES["ls_stack"], spec=dict(lc.CASES["ls_stack"]["spec"], lstm_layers=layers))))
    assert a.read_bytes() == b.read_bytes()
    with pytest.raises(ValueError):
        synth.write_final_mdl(tmp_path / "c.mdl", cases.case_spec(dict(spec=lp._lp((lp._b(form="lstmb"),)), graph="grammar", audio="zeros:0")))
    with pytest.raises(ValueError):      # (a ClipGradientComponent has no scale)
        synth.write_final_mdl(tmp_path / "d.mdl", cases.case_spec(dict(spec=lp._lp((lp._b(clipgrad=True, scale=0.9),)), graph="grammar", audio="zeros:0")))


def test_writers_of_the_two_components():
    """Field order as the reference's Write methods have it (nnet-simple-component.cc:3840-3856, 577-600), text form."""
    from rhasspy_speech_amd import synth
    w = synth.KaldiWriter(False)
    synth._w_ng_per_element_scale(w, np.array([0.5, -1.0], np.float32))
    assert w.getvalue().decode() == ("<NaturalGradientPerElementScaleComponent> <LearningRate> 0.0010000000474974513 <Params>  [ 0.5 -1.0 ]\n"
                                     "<IsGradient> F <Rank> 8 <UpdatePeriod> 10 <NumSamplesHistory> 2000.0 <Alpha> 4.0 "
                                     "</NaturalGradientPerElementScaleComponent> ")
    w = synth.KaldiWriter(False)
    synth._w_clip_gradient(w, 8)
    assert w.getvalue().decode() == ("<ClipGradientComponent> <Dim> 8 <ClippingThreshold> 30.0 <NormBasedClipping> T <SelfRepairClippedProportionThreshold> 0.009999999776482582 "
                                     "<SelfRepairTarget> 0.0 <SelfRepairScale> 1.0 <NumElementsClipped> 0 <NumElementsProcessed> 0 <NumSelfRepaired> 0 "
                                     "<NumBackpropped> 0 </ClipGradientComponent> ")
    names = [n for n, _ in synth.build_nnet(cases.case_spec(lp.CASES["lp_drop"]), np.random.default_rng(1))[1] if n.startswith("lstm1.")]
    assert names == ["lstm1.W_i.xr", "lstm1.w_i.c", "lstm1.W_f.xr", "lstm1.w_f.c", "lstm1.W_o.xr", "lstm1.w_o.c", "lstm1.W_c.xr", "lstm1.i", "lstm1.f", "lstm1.o",
                     "lstm1.g", "lstm1.h", "lstm1.dropout", "lstm1.c1", "lstm1.c2", "lstm1.m", "lstm1.c", "lstm1.W_rp.m", "lstm1.r"]
