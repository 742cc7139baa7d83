"""TDNN-LSTM models built from lstmb-layer (the cell behind a bottleneck: two LinearComponents and a ScaleAndOffsetComponent in front
of the LstmNonlinearityComponent) without a GPU: the goldens of tests/lstmb_cases.py, the float64 restatement against them and what
it takes to miss them, the recogniser of the block and its refusals, the set-up's restatement on these networks (contexts, collapsed
network, the dither rule), the reader's lowering and the planner through a stand-alone host program under the address and
undefined-behaviour sanitizers, and the synthetic model writer.  On the commit before, every load below was refused: "component type
ScaleAndOffsetComponent (node so1) is not supported by the HIP acoustic-model kernels" for the feed-forward case, and for a block
"recurrent networks are supported only as fast-lstmp-layer / fast-lstm-layer blocks (cycle at node lstm1.W_all_b_so: the
nonlinearity's first input is not an affine component node of the cycle)"."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import cases
from tests import lstm_cases as lc
from tests import lstmb_cases as lb

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in lb.CASES if n not in lb.NO_GOLDEN]
DECODED = [n for n in WITH_GOLDEN if n != "lb_len0"]
LOGLIKE_TOL = 1e-4      # the project's bound on log-likelihoods


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = lb.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _mdl(model_dir):
    return model_dir / "model" / "model" / "final.mdl"


# ------------------------------------------------------------------------------------------ goldens

def test_goldens_are_there_for_every_case():
    for name in WITH_GOLDEN:
        g = lb.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(lb.CASES[name], sort_keys=True), name      # (made from this table)
        if name == "lb_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "context", "collapsed"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                    for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "lb_stack":
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        spec = cases.case_spec(lb.CASES[name])
        assert g["input"].shape[1] == spec.feat_dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape
        fsf = lb.fsf_of(name)
        assert int(g["offline_num_frames"]) == (g["input"].shape[0] + fsf - 1) // fsf
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
    frames = {n: lb.load_golden(n)["input"].shape[0] for n in lb.LENGTHS[1:]}
    assert frames == {"lb_len1": 1, "lb_len2": 2, "lb_len25": 25, "lb_len47": 47}      # (the chunk is 24 frames)
    assert sorted(p.stem for p in lb.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in lb.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


@pytest.mark.parametrize("name", DECODED)
def test_nbest_hypotheses_are_far_enough_apart(name):
    """Adjacent n-best hypotheses differ in total cost by more than 0.02, ten times the 2e-3 cost tolerance of the GPU tests: the order
    of the list is not a matter of rounding."""
    g = lb.load_golden(name)
    for mode in ("offline", "stream"):
        total = g[f"{mode}_graph_cost"].astype(np.float64) + g[f"{mode}_acoustic_cost"]
        if len(total) > 1:
            assert np.diff(total).min() > 0.02, (name, mode, np.diff(total).min())


@pytest.mark.parametrize("name", DECODED)
def test_float64_restatement_agrees_with_the_reference(name):
    """lstmb_cases.Float64Net -- b = W_a [x; sm], g = W_b b, scale and offset through EnsureNonzero, the nonlinearity, the truncation
    scale and the descriptor's Scale() on m -- over the golden `input` rows against the reference's offline_loglikes, within the
    project's 1e-4."""
    g = lb.load_golden(name)
    ll, blocks = lb.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(blocks) == len(lb.block_dims(name))
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}")
    assert diff < LOGLIKE_TOL, diff
    if "offline_ivector" not in g.files:      # (without an extractor the streamed rows are the offline ones)
        np.testing.assert_array_equal(g["stream_loglikes"], g["offline_loglikes"])


@pytest.mark.parametrize("name", ["lb_basic", "lb_so", "lb_so_ff"])
def test_without_scale_and_offset_the_restatement_misses(name):
    """The same restatement with the ScaleAndOffsetComponent skipped does not agree: the cases can tell."""
    g = lb.load_golden(name)
    diff = float(np.abs(lb.restate(name, g, apply_scale_offset=False)[0] - g["offline_loglikes"]).max())
    print(f"{name} without scale / offset: max |restatement - reference| {diff:.4g}")
    assert diff > LOGLIKE_TOL, diff


def test_without_ensure_nonzero_the_restatement_misses():
    """lb_so with its scales as written (0, +5e-5, -5e-5 among them) instead of through cu::EnsureNonzero does not agree."""
    g = lb.load_golden("lb_so")
    diff = float(np.abs(lb.restate("lb_so", g, apply_ensure_nonzero=False)[0] - g["offline_loglikes"]).max())
    print(f"lb_so without EnsureNonzero: max |restatement - reference| {diff:.4g}")
    assert diff > LOGLIKE_TOL, diff
    s = lb.ensure_nonzero(np.array([0.0, 5e-5, -5e-5, -0.0, 1e-4, -1e-4, 0.5], np.float32))
    eps = float(np.float32(1e-4))
    assert s.tolist() == [eps, eps, -eps, eps, eps, -eps, 0.5]


# ------------------------------------------------------------------------------------------ load and describe

def _block_lines(name):
    out = []
    for k, kind, in_dim, cell, bott, delay, scale, self_scale in lb.block_dims(name):
        if kind != "lstmb":
            continue
        ct, bt = (cell + 15) // 16, (bott + 15) // 16
        lds = 16 * 4 * ((16 * ct + 4) + (16 * bt + 4))
        out.append(f"lstmb: lstm{k}.lstm_nonlin input={in_dim} cell={cell} bottleneck={bott} delay={delay} scale={scale:g} self_scale={self_scale:g} "
                   f"kernel=lstmb16x16x4<w8> rows_per_block=16 lds={lds} w_a={in_dim}+{cell} cell_tiles={ct} b_tiles={bt} grid=chains/16")
    return out


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_blocks(built, name):
    """The parent refused these directories at load.  Now they load on the host: per lstmb block one layer GEMM over W_all_a's
    feed-forward columns (bottleneck wide, no bias, no stage), an `op: lstmb` and a `lstmb:` line with the case's dims, both scales and
    what the planner chose, m_batchnorm as an elementwise op behind it; the context is the reference's."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    dims = lb.block_dims(name)
    assert [l for l in text.splitlines() if l.startswith("lstmb: ")] == _block_lines(name)
    ops = [l for l in text.splitlines() if l.startswith("op: ")]
    walks = []
    for k, kind, in_dim, cell, bott, *_r in dims:
        node = {"lstm": f"lstm{k}.lstm_nonlin", "lstmp": f"lstm{k}.c_t", "lstmb": f"lstm{k}.lstm_nonlin"}[kind]
        at = [i for i, l in enumerate(ops) if l.startswith(f"op: {kind} {node} out_dim={2 * cell} terms=1 stages=0")]
        assert len(at) == 1, ops
        if kind == "lstmb":
            assert ops[at[0] - 1].startswith(f"op: gemm lstm{k}.W_all_a.x out_dim={bott} k={in_dim} ") and " stages=0" in ops[at[0] - 1], ops
            assert ops[at[0] + 1].startswith(f"op: eltwise lstm{k}.m_batchnorm out_dim={cell} terms=1 stages=1"), ops
        walks.append(at[0])
    assert walks == sorted(walks)      # (network order: what result matrix 64 + k counts)
    assert [l.split()[1] for l in ops if l.split()[1] in ("lstm", "lstmp", "lstmb")] == [d[1] for d in dims]
    fsf = lb.fsf_of(name)
    block_ops = [l for l in ops if l.startswith("op: lstmb ")]
    if name == "lb_fsf3":        # delay 3 under factor 3 and offsets {-3, 0, 3} above: one residue class
        assert all(l.endswith(" rows=every-3") for l in block_ops)
    else:                        # (lb_fsf3_d2: delay 2 visits every class; the layers above it still run on every third row)
        assert not any("rows=every" in l for l in block_ops)
        assert ("rows=every-3" in text) == (fsf == 3)
    left, right = lb.contexts(name)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]
    if name != "lb_len0":
        assert [left, right] == lb.load_golden(name)["context"].tolist()      # (what the reference's looped decodable computed)
    if name == "lb_selfscale":
        assert " scale=0.925 self_scale=0.5 " in text
    if name == "lb_so_ff":       # outside a block the component is a scale / offset stage, here behind tdnn2's ReLU and BatchNorm
        assert not dims and "op: gemm tdnn2.affine+tdnn2.relu+tdnn2.batchnorm+so1 out_dim=32 k=96 " in text and "lstmb" not in text


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
    reference's CollapseModel (the lda transform folded into the first TDNN layer; of an lstmb block nothing collapses -- two
    LinearComponents are not combined, ScaleAndOffsetComponent is unknown to it: its lines are those synth.py wrote); with a block the
    rand() position is reported as not certain."""
    from rhasspy_speech_amd import synth
    _, certain, lines = _setup(built(name)[0], lb.fsf_of(name))
    assert certain == (1 if name == "lb_so_ff" else 0)
    assert lines == bytes(lb.load_golden(name)["collapsed"]).decode().splitlines()
    spec = cases.case_spec(lb.CASES[name])
    written = [l for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if " name=lstm" in l]
    if name != "lb_so_ff":
        assert len(written) >= 9 and [l for l in lines if " name=lstm" in l] == written


def test_default_dither_is_refused_with_the_recurrence_named(built):
    """lb_dither_default: the reference's set-up accepts the model (gen_lstmb_golden.py runs it); the rand() calls of a recurrent
    compilation are not replayed, so by the existing rule the model loads with --dither=0 only."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("lb_dither_default")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    msg = str(ei.value)
    assert "--dither=1" in msg and "cannot be derived for this network" in msg and "the network is recurrent (a cycle through node lstm1." in msg, msg


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("lb_basic")[:2]).describe()
    b = _lib.Model(*built("lb_text")[:2]).describe()
    keep = ("op:", "lstmb:", "nnet:")
    assert [l for l in a.splitlines() if l.startswith(keep)] == [l for l in b.splitlines() if l.startswith(keep)]
    assert any(l.startswith("lstmb:") for l in a.splitlines())


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


_M3, _C3 = "IfDefined(Offset(lstm1.m_trunc, -3))", "IfDefined(Offset(lstm1.c_trunc, -3))"


def _dropout_mask(text):
    """use-dropout's third input on the nonlinearity, which lstmb-layer does not have."""
    from rhasspy_speech_amd import synth
    return _add_components(text, [("lstm1.dropout_mask", lambda w: synth._w_dropout_mask(w, 3))],
                           ["component-node name=lstm1.dropout_mask component=lstm1.dropout_mask input=lstm1.dropout_mask"],
                           [(f"input=Append(lstm1.W_all_b_so, {_C3})", f"input=Append(lstm1.W_all_b_so, {_C3}, lstm1.dropout_mask)")])


def _projection_shaped(text):
    """The truncation component over Append(c, m) of two dim-ranges, as a block with a projection feeds it."""
    return _add_components(text, [], ["dim-range-node name=lstm1.c input-node=lstm1.lstm_nonlin dim-offset=0 dim=32"],
                           [("component=lstm1.cm_trunc input=lstm1.lstm_nonlin", "component=lstm1.cm_trunc input=Append(lstm1.c, lstm1.m)")])


def _block_form(text):
    """W_all_b_so in the component's block form: dim 128 over 8-long vectors."""
    from rhasspy_speech_amd import synth
    so = lambda w: synth._w_scale_and_offset(w, np.full(8, 1.25, np.float32), np.full(8, 0.5, np.float32), 128)      # noqa: E731
    return _add_components(text, [("lstm1.so_block", so)], [], [("component=lstm1.W_all_b_so input=lstm1.W_all_b", "component=lstm1.so_block input=lstm1.W_all_b")])


def _affine_in_front(text):
    """W_all_a's node on an affine component (with a bias) of the same shape."""
    from rhasspy_speech_amd import synth
    W = (np.random.default_rng(5).standard_normal((16, 64)) / 8).astype(np.float32)
    return _add_components(text, [("lstm1.W_affine", lambda w: synth._w_affine(w, "NaturalGradientAffineComponent", W, np.zeros(16, np.float32)))], [],
                           [("component-node name=lstm1.W_all_a component=lstm1.W_all_a ", "component-node name=lstm1.W_all_a component=lstm1.W_affine ")])


REFUSED = {
    "a dropout mask on the nonlinearity": (_dropout_mask, ["cycle at node lstm1.lstm_nonlin", "takes no third input, but this one reads the dropout mask lstm1.dropout_mask"]),
    "a projection's truncation input": (_projection_shaped, ["cycle at node lstm1.cm_trunc", "its input is not the nonlinearity: an lstmb-layer block has no projection"]),
    "a block-form scale / offset": (_block_form, ["cycle at node lstm1.W_all_b_so", "does not have <Scales> and <Offsets> vectors of 4 x cell-dim = 128 elements",
                                                  "its block form is not supported inside a recurrent block"]),
    "two delays": (_in_line("lstm1.W_all_a", _M3, "IfDefined(Offset(lstm1.m_trunc, -2))"), ["cycle at node lstm1.W_all_a", "two different delays in one block, 2 and 3"]),
    "a positive delay": (_in_line("lstm1.W_all_a", _M3, "IfDefined(Offset(lstm1.m_trunc, 3))"), ["cycle at node lstm1.W_all_a", "a positive delay, Offset(lstm1.m_trunc, 3)"]),
    "a delay of 9": (lambda t: _swap(_M3, "IfDefined(Offset(lstm1.m_trunc, -9))")(_swap(_C3, "IfDefined(Offset(lstm1.c_trunc, -9))")(t)),
                     ["cycle at node lstm1.lstm_nonlin", "a delay of 9 frames; the HIP kernel takes 1 to 8"]),
    "the state not through IfDefined": (_in_line("lstm1.W_all_a", _M3, "Offset(lstm1.m_trunc, -3)"), ["cycle at node lstm1.W_all_a", "is not inside IfDefined()"]),
    "an affine in W_all_a's place": (_affine_in_front, ["cycle at node lstm1.W_all_b", "its input is not a LinearComponent node of the cycle (W_all_a)"]),
    "weights of the wrong shape": (_in_line("lstm1.W_all_b", "component=lstm1.W_all_b ", "component=lstm1.W_all_a "),
                                   ["cycle at node lstm1.W_all_b", "W_all_b is 16 x 64, the block needs 4 x cell-dim rows and the bottleneck's 16 columns"]),
    "the cell state read from outside": (_swap("component=tdnn3.affine input=Append(Offset(lstm1.m_batchnorm, -3), lstm1.m_batchnorm, Offset(lstm1.m_batchnorm, 3))",
                                               "component=tdnn3.affine input=Append(Offset(lstm1.m_batchnorm, -3), lstm1.c_trunc, Offset(lstm1.m_batchnorm, 3))"),
                                         ["cycle at node lstm1.c_trunc", "the node is read from outside the block, by tdnn3.affine"]),
    "the recurrent input is c_trunc": (_in_line("lstm1.W_all_a", _M3, _C3), ["cycle at node lstm1.cm_trunc", "c_trunc and m_trunc are not the two cell-dim column ranges"]),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_cycles_that_are_no_lstmb_block_are_refused(built, tmp_path, what):
    """Anything cyclic around a ScaleAndOffsetComponent that is not exactly what lstmb-layer emits is refused at load, with the node
    and the reason, in the sentence of the other LSTM refusals: lb_text's config text with one thing changed."""
    from rhasspy_speech_amd import _lib
    edit, needles = REFUSED[what]
    dst, gd = _edited(built("lb_text"), tmp_path, edit)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    msg = str(ei.value)
    assert "recurrent networks are supported only as fast-lstmp-layer / fast-lstm-layer blocks" in msg, msg
    for needle in needles:
        assert needle in msg, (needle, msg)


def test_scale_on_the_recurrent_input_is_the_lstmb_block_s_alone(built, tmp_path):
    """Scale(s, m_trunc) loads on an lstmb block; the same on a fast block's recurrent input stays refused."""
    from rhasspy_speech_amd import _lib
    dst, gd = _edited(built("lb_text"), tmp_path / "b", _in_line("lstm1.W_all_a", _M3, "IfDefined(Offset(Scale(0.25, lstm1.m_trunc), -3))"))
    assert " self_scale=0.25 " in _lib.Model(dst, gd).describe()
    src = lc.build_case_files("ls_text", tmp_path / "src")
    dst, gd = _edited(src, tmp_path / "f", _swap("IfDefined(Offset(lstm1.r_trunc, -3))", "IfDefined(Offset(Scale(0.25, lstm1.r_trunc), -3))"))
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    msg = str(ei.value)
    assert "cycle at node lstm1.W_all" in msg and "its recurrent input is not IfDefined(Offset(node, -delay))" in msg, msg


def _refused(case, root, needle):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = cases.build_case_files(case, root)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert needle in str(ei.value), str(ei.value)


def test_sizes_beyond_the_plan_s_limits_fail_the_load(tmp_path):
    big = dict(spec=lb._lb((lb._b(cell=2304, bottleneck=16),)), graph="grammar", audio="zeros:0")
    _refused(big, tmp_path / "cell", "recurrent block lstm1.lstm_nonlin: cell dim 2304 is more than the 2048 the HIP kernel takes")
    wide = dict(spec=lb._lb((lb._b(cell=16, bottleneck=2304),)), graph="grammar", audio="zeros:0")
    _refused(wide, tmp_path / "bottleneck", "recurrent block lstm1.lstm_nonlin: bottleneck dim 2304 is more than the 2048 the HIP kernel takes")
    lds = dict(spec=lb._lb((lb._b(cell=1536, bottleneck=1024),)), graph="grammar", audio="zeros:0")
    _refused(lds, tmp_path / "lds", "(cell dim 1536 + bottleneck dim 1024, 164352 bytes) do not fit the 147456 bytes of LDS the HIP kernel keeps them in")


# ------------------------------------------------------------------------------------------ reader and planner under sanitizers

def test_reader_and_planner_under_sanitizers(built, tmp_path):
    """tests/host/lstmb_plan_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's final.mdl, runs the
    recogniser and the lowering, plans every block and compares the weight images element by element; what it prints is what
    describe() says.  A recipe-size block (cell 384, bottleneck 256), one of cell 1024 and the refused edits go through it as well:
    the recogniser's refusal paths run under the sanitizers too."""
    from rhasspy_speech_amd import _lib, synth
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "lstmb_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "lstmb_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "lstm_plan.cc",
            CSRC / "lstmb_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args, want = [], []
    for name in lb.CASES:
        args += [name, str(_mdl(built(name)[0]))]
        if name in lb.NO_GOLDEN:      # (the dither rule is the engine's, not the reader's: the network itself plans like lb_basic's)
            want += [f"{name} {l}" for l in _block_lines(name)]
        elif name == "lb_so_ff":
            want.append(f"{name} no recurrent block")
        else:
            text = _lib.Model(*built(name)[:2]).describe()
            want += [f"{name} {l}" for l in text.splitlines() if l.startswith(("lstmb: ", "lstmp: ", "lstm: "))]
    extra = {
        "x_recipe": (dict(spec=lb._lb((lb._b(cell=384, bottleneck=256, scale=0.85),)), graph="grammar", audio="zeros:0"),
                     "x_recipe lstmb: lstm1.lstm_nonlin input=32 cell=384 bottleneck=256 delay=3 scale=0.85 self_scale=1 kernel=lstmb16x16x4<w8> "
                     "rows_per_block=16 lds=41472 w_a=32+384 cell_tiles=24 b_tiles=16 grid=chains/16"),
        "x_full_size": (dict(spec=lb._lb((lb._b(cell=1024, bottleneck=256),)), graph="grammar", audio="zeros:0"),
                        "x_full_size lstmb: lstm1.lstm_nonlin input=32 cell=1024 bottleneck=256 delay=3 scale=1 self_scale=1 kernel=lstmb16x16x4<w8> "
                        "rows_per_block=16 lds=82432 w_a=32+1024 cell_tiles=64 b_tiles=16 grid=chains/16"),
        "x_cell": (dict(spec=lb._lb((lb._b(cell=2304, bottleneck=16),)), graph="grammar", audio="zeros:0"),
                   "x_cell error: nnet3: recurrent block lstm1.lstm_nonlin: cell dim 2304 is more than the 2048 the HIP kernel takes"),
        "x_plain": (dict(spec=dict(), graph="grammar", audio="zeros:0"), "x_plain no recurrent block"),
    }
    for name, (case, line) in extra.items():
        mdl = tmp_path / name / "final.mdl"
        synth.write_final_mdl(mdl, cases.case_spec(case))
        args += [name, str(mdl)]
        want.append(line)
    for i, (what, (edit, needles)) in enumerate(REFUSED.items()):
        dst, _ = _edited(built("lb_text"), tmp_path / f"refused{i}", edit)
        args += [f"r{i}", str(_mdl(dst))]
        want.append((f"r{i} error: ", needles))
    p = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    got = p.stdout.splitlines()
    # (lb_mixed's three blocks stand in the network in the order describe() prints the kinds in: lstm, lstmp, lstmb)
    assert len(got) == len(want), p.stdout
    for g, w in zip(got, want):
        if isinstance(w, tuple):
            assert g.startswith(w[0]) and all(n in g for n in w[1]), (g, w)
        else:
            assert g == w, (g, w)


# ------------------------------------------------------------------------------------------ the synthetic model writer

def test_the_writer_s_block_and_its_refusals(tmp_path):
    """A bottleneck layer writes xconfig's components and nodes in xconfig's order; form="lstmb" is not a form, and a bottleneck goes
    neither with the composed form nor with a projection.  (That specs without the key write the bytes they always wrote is pinned by
    the digest tests of the lstm / gru / pgru suites.)"""
    from rhasspy_speech_amd import synth
    spec = cases.case_spec(lb.CASES["lb_selfscale"])
    cfg, comps = synth.build_nnet(spec, np.random.default_rng(spec.seed))
    assert [n for n, _ in comps if n.startswith("lstm1.")] == ["lstm1.W_all_a", "lstm1.W_all_b", "lstm1.W_all_b_so", "lstm1.lstm_nonlin", "lstm1.cm_trunc",
                                                              "lstm1.m_batchnorm"]
    assert [l for l in cfg if " name=lstm1." in l] == [
        "component-node name=lstm1.W_all_a component=lstm1.W_all_a input=Append(tdnn2.batchnorm, IfDefined(Offset(Scale(0.5, lstm1.m_trunc), -3)))",
        "component-node name=lstm1.W_all_b component=lstm1.W_all_b input=lstm1.W_all_a",
        "component-node name=lstm1.W_all_b_so component=lstm1.W_all_b_so input=lstm1.W_all_b",
        "component-node name=lstm1.lstm_nonlin component=lstm1.lstm_nonlin input=Append(lstm1.W_all_b_so, IfDefined(Offset(lstm1.c_trunc, -3)))",
        "dim-range-node name=lstm1.m input-node=lstm1.lstm_nonlin dim-offset=32 dim=32",
        "component-node name=lstm1.cm_trunc component=lstm1.cm_trunc input=lstm1.lstm_nonlin",
        "dim-range-node name=lstm1.c_trunc input-node=lstm1.cm_trunc dim-offset=0 dim=32",
        "dim-range-node name=lstm1.m_trunc input-node=lstm1.cm_trunc dim-offset=32 dim=32",
        "component-node name=lstm1.m_batchnorm component=lstm1.m_batchnorm input=lstm1.m"]
    for bad in (dict(form="lstmb"), dict(form="composed"), dict(rec=8, nonrec=8), dict(bottleneck=0)):
        with pytest.raises(ValueError):
            synth.write_final_mdl(tmp_path / "bad.mdl", cases.case_spec(dict(spec=lb._lb((dict(lb._b(), **bad),)), graph="grammar", audio="zeros:0")))


def test_writer_of_the_scale_and_offset_component():
    """Field order as the reference's Write method has it (nnet-simple-component.cc:2381-2394), text form; the block form's <Dim>."""
    from rhasspy_speech_amd import synth
    w = synth.KaldiWriter(False)
    synth._w_scale_and_offset(w, np.array([0.5, -1.0], np.float32), np.array([0.25, 0.0], np.float32))
    assert w.getvalue().decode() == ("<ScaleAndOffsetComponent> <LearningRate> 0.0010000000474974513 <Dim> 2 <Scales>  [ 0.5 -1.0 ]\n"
                                     "<Offsets>  [ 0.25 0.0 ]\n<UseNaturalGradient> T <Rank> 20 </ScaleAndOffsetComponent> ")
    w = synth.KaldiWriter(False)
    synth._w_scale_and_offset(w, np.array([0.5, -1.0], np.float32), np.array([0.25, 0.0], np.float32), 8)
    assert "<Dim> 8 <Scales>  [ 0.5 -1.0 ]" in w.getvalue().decode()
