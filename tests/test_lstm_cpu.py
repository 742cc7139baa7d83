"""TDNN-LSTM models (recurrent blocks of LstmNonlinearityComponent, BackpropTruncationComponent, DropoutMaskComponent) without a
GPU: the goldens of tests/lstm_cases.py, the float64 restatement against them, the block recogniser and its refusals, the set-up's
restatement on recurrent networks (contexts, collapsed network, the dither rule), the load-time planner through a stand-alone host
program under the address and undefined-behaviour sanitizers, and the synthetic model writer."""
import ctypes as C
import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import cases
from tests import lstm_cases as lc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in lc.CASES if n not in lc.NO_GOLDEN]
DECODED = [n for n in WITH_GOLDEN if n != "ls_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = lc.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _mdl(model_dir):
    return model_dir / "model" / "model" / "final.mdl"


# ------------------------------------------------------------------------------------------ goldens

def test_goldens_are_there_for_every_case():
    for name in WITH_GOLDEN:
        g = lc.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(lc.CASES[name], sort_keys=True), name      # (made from this table)
        if name == "ls_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "context", "collapsed"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                    for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "ls_stack":
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        spec = cases.case_spec(lc.CASES[name])
        assert g["input"].shape[1] == spec.feat_dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape
        fsf = lc.fsf_of(name)
        assert int(g["offline_num_frames"]) == (g["input"].shape[0] + fsf - 1) // fsf
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
    frames = {n: lc.load_golden(n)["input"].shape[0] for n in lc.LENGTHS[1:]}
    assert frames == {"ls_len1": 1, "ls_len2": 2, "ls_len25": 25, "ls_len47": 47}      # (the chunk is 24 frames)
    assert sorted(p.stem for p in lc.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in lc.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


@pytest.mark.parametrize("name", DECODED)
def test_nbest_hypotheses_are_far_enough_apart(name):
    """Adjacent n-best hypotheses differ in total cost by more than 0.02, ten times the 2e-3 cost tolerance of the GPU tests: the order
    of the list is not a matter of rounding."""
    g = lc.load_golden(name)
    for mode in ("offline", "stream"):
        total = g[f"{mode}_graph_cost"].astype(np.float64) + g[f"{mode}_acoustic_cost"]
        if len(total) > 1:
            assert np.diff(total).min() > 0.02, (name, mode, np.diff(total).min())


@pytest.mark.parametrize("name", DECODED)
def test_float64_restatement_agrees_with_the_reference(name):
    """lstm_cases.Float64Net -- the recurrence of CpuComputeLstmNonlinearity over the golden `input` rows, chains started where the
    block's feed-forward input first exists, the state scaled by the truncation component -- against the reference's
    offline_loglikes, within 2.5e-5: a quarter of the device bound, so that the reference's own FP32 rounding does not consume it.
    Measured when the goldens were made: 1.6e-07 (ls_len1) to 1.1e-06 (ls_odd, ls_stack)."""
    g = lc.load_golden(name)
    ll, blocks = lc.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(blocks) == len(lc.block_dims(name))
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}")
    assert diff < 2.5e-5, diff
    if "offline_ivector" not in g.files:      # (without an extractor the streamed rows are the offline ones)
        np.testing.assert_array_equal(g["stream_loglikes"], g["offline_loglikes"])


# ------------------------------------------------------------------------------------------ load and describe

def _lstm_lines(name):
    out = []
    for k, (in_dim, cell, rec, nonrec, delay, scale, mask) in enumerate(lc.block_dims(name), start=1):
        rec_dim = rec if rec else cell
        lds = 16 * 4 * (2 * ((rec_dim + 15) // 16 * 16 + 4) + (((cell + 15) // 16 * 16 + 4) if rec else 0))
        out.append(f"lstm: lstm{k}.lstm_nonlin input={in_dim} cell={cell} rec={rec} nonrec={nonrec} delay={delay} scale={scale:g} dropout_mask={mask} "
                   f"kernel=lstm16x16x4<w8> rows_per_block=16 lds={lds} w_all={in_dim}+{rec_dim} cell_tiles={(cell + 15) // 16} "
                   f"out_tiles={(rec + nonrec + 15) // 16} grid=chains/16")
    return out


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_blocks(built, name):
    """The parent refused these directories at load ("recurrent networks are not supported (cycle at node ...)").  Now they load on
    the host: per block a layer GEMM over W_all's feed-forward columns, an `op: lstm` and a `lstm:` line with the case's dims and
    what the planner chose; the context is the reference's (ComputeSimpleNnetContext ignores the recurrent connections)."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    dims = lc.block_dims(name)
    assert [l for l in text.splitlines() if l.startswith("lstm: ")] == _lstm_lines(name)
    ops = [l for l in text.splitlines() if l.startswith("op: ")]
    for k, (in_dim, cell, *_r) in enumerate(dims, start=1):
        at = [i for i, l in enumerate(ops) if l.startswith(f"op: lstm lstm{k}.lstm_nonlin out_dim={2 * cell} terms=1 stages=0")]
        assert len(at) == 1 and ops[at[0] - 1].startswith(f"op: gemm lstm{k}.W_all.x out_dim={4 * cell} k={in_dim} "), ops
    fsf = lc.fsf_of(name)
    lstm_ops = [l for l in ops if l.startswith("op: lstm ")]
    if name == "ls_fsf3":        # delay 3 under factor 3 and offsets {-3, 0, 3} above: one residue class
        assert all(l.endswith(" rows=every-3") for l in lstm_ops)
    else:                        # (ls_fsf3_d2: delay 2 visits every class; the layers above it still run on every third row)
        assert not any("rows=every" in l for l in lstm_ops)
        assert ("rows=every-3" in text) == (fsf == 3)
    left, right = lc.contexts(name)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]
    if name != "ls_len0":
        assert [left, right] == lc.load_golden(name)["context"].tolist()      # (what the reference's looped decodable computed)
    if name == "ls_stack":       # BatchNorm on rp: an elementwise op of its own, the block's buffers stay as the block wrote them
        assert "op: eltwise lstm2.rp_batchnorm out_dim=24 terms=1 stages=1\n" in text


def test_mfcc_model_describes_itself_as_before(tmp_path):
    from rhasspy_speech_amd import _lib, synth
    spec = synth.tiny_spec()
    synth.write_model_dir(tmp_path / "model", spec)
    synth.make_grammar_graph(tmp_path / "graph", spec)
    text = _lib.Model(tmp_path / "model", tmp_path / "graph").describe()
    assert "lstm" not in text
    assert [l.split()[1] for l in text.splitlines() if l.startswith("op: ")] == ["gemm"] * text.count("op: ")


def _setup(md, fsf):
    from rhasspy_speech_amd import _lib
    lib = _lib.load_library()
    lib.rs_nnet3_setup_subsampled.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    n, cert, buf = C.c_int64(), C.c_int32(), C.create_string_buffer(1 << 16)
    assert lib.rs_nnet3_setup_subsampled(str(_mdl(md)).encode(), 24, fsf, C.byref(n), C.byref(cert), buf, len(buf)) == 0
    return n.value, cert.value, buf.value.decode().splitlines()


@pytest.mark.parametrize("name", DECODED)
def test_setup_accepts_recurrent_networks_and_leaves_the_reference_s_network(built, name):
    """rs_nnet3_setup (csrc/nnet3_setup.cc, host code) on a recurrent network: the context search, the collapser and the five-request
    walk run as for every model; the collapsed network is the one rs-dump printed after the reference's CollapseModel (the lda
    transform folded into the first TDNN layer; of a block nothing collapses: its lines are those synth.py wrote); the rand()
    position is reported as not certain."""
    from rhasspy_speech_amd import synth
    _, certain, lines = _setup(built(name)[0], lc.fsf_of(name))
    assert certain == 0
    assert lines == bytes(lc.load_golden(name)["collapsed"]).decode().splitlines()
    assert any(l.startswith("component-node name=tdnn1.affine component=lda.tdnn1.affine input=Append(Offset(input, -1), input, Offset(input, 1)") for l in lines[:3])
    spec = cases.case_spec(lc.CASES[name])
    written = [l for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if " name=lstm" in l]
    assert len(written) >= 6 and [l for l in lines if " name=lstm" in l] == written


def test_default_dither_is_refused_with_the_recurrence_named(built):
    """ls_dither_default: the reference's set-up accepts the model (gen_lstm_golden.py runs it); the rand() calls of a recurrent
    compilation are not replayed, so by the existing rule the model loads with --dither=0 only."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("ls_dither_default")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    msg = str(ei.value)
    assert "--dither=1" in msg and "cannot be derived for this network" in msg and "the network is recurrent (a cycle through node lstm1." in msg, msg


def _edited(built, tmp_path, edit):
    """ls_text's model directory (text form) with its final.mdl passed through `edit`."""
    md, gd, _, _ = built("ls_text")
    dst = tmp_path / "model"
    shutil.copytree(md, dst)
    for f in (dst / "model" / "online" / "conf").iterdir():
        f.write_text(f.read_text().replace(str(md), str(dst)))
    text = _mdl(dst).read_text()
    new = edit(text)
    assert new != text
    _mdl(dst).write_text(new)
    return dst, gd


def _swap(old, new):
    def edit(text):
        assert text.count(old) == 1, (old, text.count(old))
        return text.replace(old, new)
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


def _non_fast_lstmp(text):
    """A cell in the manner of the non-"fast" lstmp-layer (xconfig/lstm.py: XconfigLstmpLayer): gates from Sigmoid / Tanh components
    multiplied by an ElementwiseProductComponent, the product fed back through IfDefined(Offset(., -3))."""
    from rhasspy_speech_amd import synth
    rng = np.random.default_rng(3)
    W = (rng.standard_normal((32, 64)) / 8).astype(np.float32)
    comps = [("nf.W", lambda w: synth._w_affine(w, "NaturalGradientAffineComponent", W, np.zeros(32, np.float32))),
             ("nf.sig", lambda w: synth._w_nonlinear(w, "SigmoidComponent", 32)),
             ("nf.tanh", lambda w: synth._w_nonlinear(w, "TanhComponent", 32)),
             ("nf.prod", lambda w: w.token("<ElementwiseProductComponent>").token("<InputDim>").i32(64).token("<OutputDim>").i32(32)
              .token("</ElementwiseProductComponent>"))]
    nodes = ["component-node name=nf.W component=nf.W input=Append(tdnn3.batchnorm, IfDefined(Offset(nf.m, -3)))",
             "component-node name=nf.i component=nf.sig input=nf.W",
             "component-node name=nf.g component=nf.tanh input=nf.W",
             "component-node name=nf.m component=nf.prod input=Append(nf.i, nf.g)"]
    rewire = [("component=prefinal-chain.affine input=tdnn3.batchnorm", "component=prefinal-chain.affine input=nf.m")]
    return _add_components(text, comps, nodes, rewire)


REFUSED = {
    "positive delay": (_swap("IfDefined(Offset(lstm1.r_trunc, -3))", "IfDefined(Offset(lstm1.r_trunc, 3))"),
                       ["cycle at node lstm1.W_all", "a positive delay, Offset(lstm1.r_trunc, 3)"]),
    "two delays": (_swap("IfDefined(Offset(lstm1.r_trunc, -3))", "IfDefined(Offset(lstm1.r_trunc, -2))"),
                   ["cycle at node lstm1.W_all", "two different delays in one block, 2 and 3"]),
    "delay beyond the kernel": (lambda t: _swap("IfDefined(Offset(lstm1.r_trunc, -3))", "IfDefined(Offset(lstm1.r_trunc, -9))")(
        _swap("IfDefined(Offset(lstm1.c_trunc, -3))", "IfDefined(Offset(lstm1.c_trunc, -9))")(t)),
                                ["cycle at node lstm1.lstm_nonlin", "a delay of 9 frames; the HIP kernel takes 1 to 8"]),
    "the non-fast layer": (_non_fast_lstmp, ["cycle at node nf.", "the cycle has no LstmNonlinearityComponent", "lstmp-layer"]),
    "a cycle that is not a block": (_swap("component=lstm1.W_rp input=lstm1.m", "component=lstm1.W_rp input=Sum(lstm1.m, IfDefined(Offset(lstm1.c, -1)))"),
                                    ["cycle at node lstm1.rp", "the projection's input is not m"]),
    "the state not through IfDefined": (_swap("IfDefined(Offset(lstm1.c_trunc, -3))", "Offset(lstm1.c_trunc, -3)"),
                                        ["cycle at node lstm1.lstm_nonlin", "is not inside IfDefined()"]),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_cycles_that_are_no_fast_lstm_block_are_refused(built, tmp_path, what):
    """Anything cyclic that is not what fast-lstmp-layer / fast-lstm-layer emit stays refused at load, with the node and the reason:
    ls_text's config text with one thing changed."""
    from rhasspy_speech_amd import _lib
    edit, needles = REFUSED[what]
    dst, gd = _edited(built, tmp_path, edit)
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


def test_sizes_beyond_the_kernel_s_limits_fail_the_load(tmp_path):
    big = dict(spec=lc._ls((lc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(big, tmp_path / "cell", "recurrent block lstm1.lstm_nonlin: cell dim 2304 is more than the 2048 the HIP kernel takes")
    lds = dict(spec=lc._ls((lc._b(cell=1200, rec=0, nonrec=0),)), graph="grammar", audio="zeros:0")
    _refused(lds, tmp_path / "lds", "do not fit the 147456 bytes of LDS the HIP kernel keeps them in")


def test_a_truncation_scale_outside_a_block_is_honoured(built, tmp_path):
    """BackpropTruncationComponent::Propagate multiplies by <Scale> wherever the component stands (it was an identity before): the
    block's scale is in its `lstm:` line, and a copy of the component used as an ordinary layer becomes a scale stage."""
    from rhasspy_speech_amd import _lib, synth
    text = _lib.Model(*built("ls_decay")[:2]).describe()
    assert " delay=3 scale=0.925 " in [l for l in text.splitlines() if l.startswith("lstm: ")][0]

    def edit(scale):
        return lambda t: _add_components(t, [("bt", lambda w: synth._w_backprop_truncation(w, 32, scale, 1))],
                                         ["component-node name=bt component=bt input=tdnn3.batchnorm"],
                                         [("component=prefinal-chain.affine input=tdnn3.batchnorm", "component=prefinal-chain.affine input=bt")])
    for scale, stages in ((0.5, 3), (1.0, 2)):      # (at scale 1 nothing changes: no stage)
        dst, gd = _edited(built, tmp_path / str(stages), edit(scale))
        assert f"op: gemm tdnn3.affine+tdnn3.relu+tdnn3.batchnorm+bt out_dim=32 k=48 segs=[6:-3:16][6:0:16][6:3:16] stages={stages}\n" in _lib.Model(dst, gd).describe()


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("ls_basic")[:2]).describe()
    b = _lib.Model(*built("ls_text")[:2]).describe()
    keep = ("op:", "lstm:", "nnet:")
    assert [l for l in a.splitlines() if l.startswith(keep)] == [l for l in b.splitlines() if l.startswith(keep)]


# ------------------------------------------------------------------------------------------ the planner under sanitizers

def test_reader_and_planner_under_sanitizers(built, tmp_path):
    """tests/host/lstm_plan_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's final.mdl, compiles
    the network, plans every block and walks plan and weight images the way the kernel does; what it prints is what describe() says."""
    from rhasspy_speech_amd import _lib, synth
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "lstm_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "lstm_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "lstm_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args, want = [], []
    for name in lc.CASES:
        args += [name, str(_mdl(built(name)[0]))]
        if name in lc.NO_GOLDEN:      # (the dither rule is the engine's, not the reader's: the network itself plans like ls_basic's)
            want += [f"{name} {l}" for l in _lstm_lines(name)]
        else:
            text = _lib.Model(*built(name)[:2]).describe()
            want += [f"{name} {l}" for l in text.splitlines() if l.startswith("lstm: ")]
    extra = {
        "x_full_size": (dict(spec=lc._ls((lc._b(cell=1024, rec=256, nonrec=256),)), graph="grammar", audio="zeros:0"),
                        "x_full_size lstm: lstm1.lstm_nonlin input=32 cell=1024 rec=256 nonrec=256 delay=3 scale=1 dropout_mask=0 kernel=lstm16x16x4<w8> "
                        "rows_per_block=16 lds=99072 w_all=32+256 cell_tiles=64 out_tiles=32 grid=chains/16"),
        "x_cell": (dict(spec=lc._ls((lc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0"),
                   "x_cell error: nnet3: recurrent block lstm1.lstm_nonlin: cell dim 2304 is more than the 2048 the HIP kernel takes"),
        "x_plain": (dict(spec=dict(), graph="grammar", audio="zeros:0"), "x_plain no recurrent block"),
    }
    for name, (case, line) in extra.items():
        mdl = tmp_path / name / "final.mdl"
        synth.write_final_mdl(mdl, cases.case_spec(case))
        args += [name, str(mdl)]
        want.append(line)
    p = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    assert p.stdout.splitlines() == want, p.stdout


# ------------------------------------------------------------------------------------------ the synthetic model writer

# sha256 over (relative path, bytes) of every file synth.write_model_dir(tiny_spec(**kw)) wrote on the commit before lstm_layers was
# added to ModelSpec (the directory's own path replaced by <ROOT>): the table of tests/test_conv_cpu.py plus a convolutional spec
PARENT_MODEL_SHA256 = {
    "tiny": (dict(), "09676d237fabef783f6ed1e813df44cbff9e1987a34446a24e54824537985ee5"),
    "tiny_text": (dict(binary=False), "e85b59f74ae8b5e856d4ebba742ebb1382d4535e70766baead3a978a0724bfc0"),
    "tiny_tdnnf_noiv": (dict(tdnnf=True, ivector_dim=0, seed=5), "004b2430aede82a792cdefb0565eb5ab434d3b9c3dad894ee07dfefd7665fb21"),
    "tiny_priors_softmax": (dict(with_priors=True, with_log_softmax=True, context="triphone"),
                            "aca5be905bdb0384f3a0ec033d85051a65f06277dc0d15cd7c0c660b776371bd"),
}


@pytest.mark.parametrize("key", list(PARENT_MODEL_SHA256))
def test_existing_specs_write_the_bytes_they_always_wrote(tmp_path, key):
    from rhasspy_speech_amd import synth
    kw, want = PARENT_MODEL_SHA256[key]
    assert synth.tiny_spec(**kw).lstm_layers == ()
    synth.write_model_dir(tmp_path / "m", synth.tiny_spec(**kw))
    h = hashlib.sha256()
    for f in sorted((tmp_path / "m").rglob("*")):
        if f.is_file():
            h.update(str(f.relative_to(tmp_path / "m")).encode() + b"\0" + f.read_bytes().replace(str(tmp_path).encode(), b"<ROOT>"))
    assert h.hexdigest() == want


def test_writers_of_the_three_components():
    """Field order as the reference's Write methods have it (nnet-combined-component.cc:1019-1057, nnet-general-component.cc:932-955,
    1499-1510), text form."""
    from rhasspy_speech_amd import synth
    w = synth.KaldiWriter(False)
    synth._w_backprop_truncation(w, 40, 0.925, 3)
    assert w.getvalue().decode() == ("<BackpropTruncationComponent> <Dim> 40 <Scale> 0.925000011920929 <ClippingThreshold> 30.0 <ZeroingThreshold> 15.0 "
                                     "<ZeroingInterval> 20 <RecurrenceInterval> 3 <NumElementsClipped> 0.0 <NumElementsZeroed> 0.0 "
                                     "<NumElementsProcessed> 0.0 <NumZeroingBoundaries> 0.0 </BackpropTruncationComponent> ")
    w = synth.KaldiWriter(False)
    synth._w_dropout_mask(w, 3)
    assert w.getvalue().decode() == "<DropoutMaskComponent> <OutputDim> 3 <DropoutProportion> 0.0 <TestMode> F </DropoutMaskComponent> "
    w = synth.KaldiWriter(True)
    synth._w_lstm_nonlinearity(w, np.zeros((3, 2), np.float32), True)
    b = w.getvalue()
    order = [b"<LstmNonlinearityComponent> ", b"<LearningRate> ", b"<Params> ", b"<ValueAvg> ", b"<DerivAvg> ", b"<SelfRepairConfig> ", b"<SelfRepairProb> ",
             b"<UseDropout> T", b"<Count> ", b"</LstmNonlinearityComponent> "]
    at = [b.index(t) for t in order]
    assert at == sorted(at)
    w = synth.KaldiWriter(True)
    synth._w_lstm_nonlinearity(w, np.zeros((3, 2), np.float32), False)
    assert b"<UseDropout>" not in w.getvalue()      # (written only when true)
    assert synth.lstm_layer_dims(dict(cell=24)) == (24, 0, 0, 24) and synth.lstm_layer_dims(dict(cell=32, rec=8, nonrec=8)) == (32, 8, 8, 16)
    with pytest.raises(ValueError):
        synth.lstm_layer_dims(dict(cell=32, rec=8))
