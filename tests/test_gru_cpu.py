"""TDNN-OPGRU models (recurrent blocks of OutputGruNonlinearityComponent: fast-opgru-layer / fast-norm-opgru-layer) without a GPU:
the goldens of tests/gru_cases.py, the float64 restatement against them, the block recogniser and its refusals, the set-up's
restatement (contexts, collapsed network, the dither rule), the load-time planner through a stand-alone host program under the
address and undefined-behaviour sanitizers, and the synthetic model writer."""
import ctypes as C
import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import cases
from tests import gru_cases as gc
from tests import lstm_cases as lc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in gc.CASES if n not in gc.NO_GOLDEN]
DECODED = [n for n in WITH_GOLDEN if n != "gr_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = gc.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _mdl(model_dir):
    return model_dir / "model" / "model" / "final.mdl"


# ------------------------------------------------------------------------------------------ goldens

def test_goldens_are_there_for_every_case():
    for name in WITH_GOLDEN:
        g = gc.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(gc.CASES[name], sort_keys=True), name      # (made from this table)
        if name == "gr_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "context", "collapsed"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                    for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "gr_stack":
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        spec = cases.case_spec(gc.CASES[name])
        assert g["input"].shape[1] == spec.feat_dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape
        fsf = gc.fsf_of(name)
        assert int(g["offline_num_frames"]) == (g["input"].shape[0] + fsf - 1) // fsf
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
    frames = {n: gc.load_golden(n)["input"].shape[0] for n in gc.LENGTHS[1:]}
    assert frames == {"gr_len1": 1, "gr_len2": 2, "gr_len25": 25, "gr_len47": 47}      # (the chunk is 24 frames)
    assert sorted(p.stem for p in gc.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in gc.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


@pytest.mark.parametrize("name", DECODED)
def test_nbest_hypotheses_are_far_enough_apart(name):
    """Adjacent n-best hypotheses differ in total cost by more than 0.02, ten times the 2e-3 cost tolerance of the GPU tests: the order
    of the list is not a matter of rounding.  A condition on the reference's output alone (the audio seeds were chosen for it)."""
    g = gc.load_golden(name)
    for mode in ("offline", "stream"):
        total = g[f"{mode}_graph_cost"].astype(np.float64) + g[f"{mode}_acoustic_cost"]
        if len(total) > 1:
            assert np.diff(total).min() > 0.02, (name, mode, np.diff(total).min())


@pytest.mark.parametrize("name", DECODED)
def test_float64_restatement_agrees_with_the_reference(name):
    """gru_cases.Float64Net -- OutputGruNonlinearityComponent::Propagate over the golden `input` rows between the sigmoids, the product,
    W_y, NormalizePerRow and the truncation scale, chains started where the block's feed-forward input first exists -- against the
    reference's offline_loglikes, within 2.5e-5: a quarter of the device bound (the bound of test_lstm_cpu.py).  Measured when the
    goldens were made: 1.3e-07 (gr_len2) to 1.9e-06 (gr_norm_drop); every other case below 9.4e-07."""
    g = gc.load_golden(name)
    ll, blocks = gc.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(blocks) == len(gc.block_dims(name))
    for rows, (_kind, _k, _in, out_dim, _layer) in zip(blocks, gc.block_dims(name)):
        assert rows.shape == (g["input"].shape[0], out_dim)
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}")
    assert diff < 2.5e-5, diff
    if "offline_ivector" not in g.files:      # (without an extractor the streamed rows are the offline ones)
        np.testing.assert_array_equal(g["stream_loglikes"], g["offline_loglikes"])


# ------------------------------------------------------------------------------------------ load and describe

def _gru_lines(name):
    """The `gru:` lines of the case by the planner's rules: k extents rounded up to 16, LDS pitches of k + 4 floats, two tiles of s
    rows and one of c . o rows for 16 chains."""
    out = []
    for kind, k, in_dim, _out, layer in gc.block_dims(name):
        if kind != "gru":
            continue
        cell, rec, nonrec = int(layer["cell"]), int(layer["rec"]), int(layer["nonrec"])
        lds = 16 * 4 * (2 * ((rec + 15) // 16 * 16 + 4) + ((cell + 15) // 16 * 16 + 4))
        out.append(f"gru: gru{k}.gru_nonlin_t input={in_dim} cell={cell} rec={rec} nonrec={nonrec} delay={int(layer.get('delay', 3))} "
                   f"scale={float(layer.get('scale', 1.0)):g} norm={int(bool(layer.get('norm', False)))} dropout={int(bool(layer.get('dropout', False)))} "
                   f"kernel=gru16x16x4<w8> rows_per_block=16 lds={lds} w_zo={in_dim}+{rec} cell_tiles={(cell + 15) // 16} "
                   f"out_tiles={(rec + nonrec + 15) // 16} grid=chains/16")
    return out


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_blocks(built, name):
    """The parent refused these directories at load ("recurrent networks are supported only as fast-lstmp-layer / fast-lstm-layer
    blocks").  Now they load on the host: per block ONE layer GEMM over the feed-forward columns of W_z, W_o and W_hpart (3 cell
    rows), an `op: gru` and a `gru:` line with the case's dims and what the planner chose; the context is the reference's."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    assert [l for l in text.splitlines() if l.startswith("gru: ")] == _gru_lines(name)
    ops = [l for l in text.splitlines() if l.startswith("op: ")]
    rec_ops = [l for l in ops if l.startswith(("op: lstm ", "op: gru "))]
    dims = gc.block_dims(name)
    assert [l.split()[1:3] for l in rec_ops] == [[kind, f"{kind}{k}.{'gru_nonlin_t' if kind == 'gru' else 'lstm_nonlin'}"] for kind, k, *_r in dims]
    for kind, k, in_dim, _out, layer in dims:
        if kind != "gru":
            continue
        cell = int(layer["cell"])
        at = [i for i, l in enumerate(ops) if l.startswith(f"op: gru gru{k}.gru_nonlin_t out_dim={2 * cell} terms=1 stages=0")]
        assert len(at) == 1 and ops[at[0] - 1].startswith(f"op: gemm gru{k}.gru_nonlin_t.x out_dim={3 * cell} k={in_dim} "), ops
        if layer.get("norm", False):     # BatchNorm on y: an elementwise op of its own, the block's rows stay as the block wrote them
            assert f"op: eltwise gru{k}.y_t out_dim={int(layer['rec']) + int(layer['nonrec'])} terms=1 stages=1" in "\n".join(ops)
    fsf = gc.fsf_of(name)
    if name == "gr_fsf3":        # delay 3 under factor 3 and offsets {-3, 0, 3} above: one residue class
        assert all(l.endswith(" rows=every-3") for l in rec_ops)
    else:                        # (gr_fsf3_d2: delay 2 visits every class; the layers above it still run on every third row)
        assert not any("rows=every" in l for l in rec_ops)
        assert ("rows=every-3" in text) == (fsf == 3)
    left, right = gc.contexts(name)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]
    if name != "gr_len0":
        assert [left, right] == gc.load_golden(name)["context"].tolist()      # (what the reference's looped decodable computed)


# sha256 of describe()'s structural lines (everything but the two state lines `layer_gemm:` and `arenas:`) on the commit before the
# GRU blocks: lstm_cases' ls_stack (two LSTM blocks, iVector) and the tiny MFCC TDNN
PARENT_DESCRIBE_SHA256 = {
    "ls_stack": "2b0ddf5cb48f1008ca7fee14d0314c1957b2d82eb2c226e0824d8878c70c8c2f",
    "tiny": "c1cee302a647940be01e5cb7f8ac3f9d21f47bb69b4d9e2a5592198c05603733",
}


def _structure_sha(text):
    keep = [l for l in text.splitlines() if not l.startswith(("layer_gemm:", "arenas:"))]
    return hashlib.sha256("\n".join(keep).encode()).hexdigest()


def test_lstm_and_tdnn_models_describe_themselves_as_before(tmp_path):
    from rhasspy_speech_amd import _lib, synth
    md, gd, _, _ = lc.build_case_files("ls_stack", tmp_path / "ls")
    text = _lib.Model(md, gd).describe()
    assert "gru" not in text and text.count("\nlstm: ") == 2
    assert _structure_sha(text.replace(str(tmp_path), "<ROOT>")) == PARENT_DESCRIBE_SHA256["ls_stack"]
    spec = synth.tiny_spec()
    synth.write_model_dir(tmp_path / "model", spec)
    synth.make_grammar_graph(tmp_path / "graph", spec)
    text = _lib.Model(tmp_path / "model", tmp_path / "graph").describe()
    assert "gru" not in text and "lstm" not in text
    assert _structure_sha(text.replace(str(tmp_path), "<ROOT>")) == PARENT_DESCRIBE_SHA256["tiny"]


def _setup(md, fsf):
    from rhasspy_speech_amd import _lib
    lib = _lib.load_library()
    lib.rs_nnet3_setup_subsampled.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    n, cert, buf = C.c_int64(), C.c_int32(), C.create_string_buffer(1 << 16)
    assert lib.rs_nnet3_setup_subsampled(str(_mdl(md)).encode(), 24, fsf, C.byref(n), C.byref(cert), buf, len(buf)) == 0
    return n.value, cert.value, buf.value.decode().splitlines()


@pytest.mark.parametrize("name", DECODED)
def test_setup_leaves_the_reference_s_network(built, name):
    """rs_nnet3_setup on a network with GRU blocks: the collapsed network is the one rs-dump printed after the reference's
    CollapseModel.  Of a block nothing collapses -- its lines are those synth.py wrote; in particular the norm variant's BatchNorm
    stays a node of its own behind W_y (y_t_tmp has two readers, and the affine / scale collapser does not take a BatchNorm) -- and
    the rand() position is reported as not certain."""
    from rhasspy_speech_amd import synth
    _, certain, lines = _setup(built(name)[0], gc.fsf_of(name))
    assert certain == 0
    assert lines == bytes(gc.load_golden(name)["collapsed"]).decode().splitlines()
    spec = cases.case_spec(gc.CASES[name])
    written = [l for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if " name=gru" in l]
    assert len(written) >= 11 and [l for l in lines if " name=gru" in l] == written
    if any(layer.get("norm", False) for layer in spec.gru_layers):
        assert any(".y_t component=" in l and ".batchnorm input=" in l and l.endswith(".y_t_tmp") for l in lines)


def test_default_dither_is_refused_with_the_recurrence_named(built):
    """gr_dither_default: the reference's set-up accepts the model (gen_gru_golden.py runs it); the rand() calls of a recurrent
    compilation are not replayed, so by the existing rule the model loads with --dither=0 only."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("gr_dither_default")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    msg = str(ei.value)
    assert "--dither=1" in msg and "cannot be derived for this network" in msg and "the network is recurrent (a cycle through node gru1." in msg, msg


# ------------------------------------------------------------------------------------------ refusals

_NORM_TEXT = dict(spec=gc._gr((gc._b(norm=True),), binary=False), graph="grammar", audio="zeros:0")


def _edited(src, tmp_path, edit):
    """A model directory (text form) with its final.mdl passed through `edit`."""
    md, gd = src
    dst = tmp_path / "model"
    shutil.copytree(md, dst)
    for f in (dst / "model" / "online" / "conf").iterdir():
        f.write_text(f.read_text().replace(str(md), str(dst)))
    text = _mdl(dst).read_text()
    new = edit(text)
    assert new != text
    _mdl(dst).write_text(new)
    return dst, gd


def _swap(*pairs, count=1):
    def edit(text):
        for old, new in pairs:
            assert text.count(old) == count, (old, text.count(old))
            text = text.replace(old, new)
        return text
    return edit


def _add_nodes(nodes, *pairs):
    """Appends config lines to a text model and applies the (old, new) replacements."""
    def edit(text):
        text = _swap(*pairs)(text)
        head, rest = text.split("\n\n<NumComponents> ", 1)
        return head + "\n" + "\n".join(nodes) + "\n\n<NumComponents> " + rest
    return edit


_S3, _C3 = "IfDefined(Offset(gru1.s_t, -3))", "IfDefined(Offset(gru1.c_t, -3))"
_ZPRE = "component-node name=gru1.z_t_pre component=gru1.W_z.xs input=Append(tdnn2.batchnorm, " + _S3 + ")"
_OPRE = "component-node name=gru1.o_t_pre component=gru1.W_o.xs input=Append(tdnn2.batchnorm, " + _S3 + ")"
_HPART = "component-node name=gru1.hpart_t component=gru1.W_hpart.x input=tdnn2.batchnorm"
_X2 = "Sum(tdnn2.batchnorm, gru1.c_t)"

REFUSED = {
    "a positive delay": ("basic", _swap((_C3, "IfDefined(Offset(gru1.c_t, 3))")),
                         ["cycle at node gru1.gru_nonlin_t", "a positive delay, Offset(gru1.c_t, 3)"]),
    "different delays": ("basic", _swap((_ZPRE, _ZPRE.replace("-3", "-2"))),
                         ["cycle at node gru1.z_t_pre", "two different delays in one block, 2 and 3"]),
    "a delay outside 1..8": ("basic", lambda t: _swap((_C3, _C3.replace("-3", "-9")))(_swap((_S3, _S3.replace("-3", "-9")), count=2)(t)),
                             ["cycle at node gru1.gru_nonlin_t", "a delay of 9 frames; the HIP kernel takes 1 to 8"]),
    "a state not inside IfDefined": ("basic", _swap((_C3, "Offset(gru1.c_t, -3)")),
                                     ["cycle at node gru1.gru_nonlin_t", "its recurrent input gru1.c_t is not inside IfDefined()"]),
    "a feed-forward input that reads the cycle": ("basic", _swap((_ZPRE, _ZPRE.replace("tdnn2.batchnorm", _X2)), (_OPRE, _OPRE.replace("tdnn2.batchnorm", _X2)),
                                                                  (_HPART + "\n", _HPART.replace("tdnn2.batchnorm", _X2) + "\n")),
                                                  ["cycle at node gru1.z_t_pre", "its feed-forward input reads gru1.c_t, a node of the cycle"]),
    "a recurrent dim the weights do not have": ("basic", _swap(("dim-range-node name=gru1.s_t_preclip input-node=gru1.y_t dim-offset=0 dim=8",
                                                                "dim-range-node name=gru1.s_t_preclip input-node=gru1.y_t dim-offset=0 dim=4"),
                                                               ("<BackpropTruncationComponent> <Dim> 8 ", "<BackpropTruncationComponent> <Dim> 4 ")),
                                                ["cycle at node gru1.z_t_pre", "its weights are 32 x 40", "the feed-forward input's 32 + the recurrent input's 4 columns"]),
    "a node with two roles": ("basic", _swap(("input=Append(gru1.c_t, gru1.o_t)", "input=Append(gru1.c_t, gru1.z_t)")),
                              ["cycle at node gru1.gru_nonlin_t", "a node has two roles in the block"]),
    "a second nonlinearity": ("basic", _add_nodes(["component-node name=gru1.nl2 component=gru1.gru_nonlin input=Append(gru1.z_t, gru1.hpart_t, " + _C3 + ")",
                                                   "dim-range-node name=gru1.c2 input-node=gru1.nl2 dim-offset=32 dim=32"],
                                                  ("input=Append(gru1.c_t, gru1.o_t)", "input=Append(gru1.c2, gru1.o_t)")),
                              ["cycle at node gru1.", "a second OutputGruNonlinearityComponent in one cycle"]),
    "GruNonlinearityComponent": ("basic", _swap(("<OutputGruNonlinearityComponent>", "<GruNonlinearityComponent>"),
                                                ("</OutputGruNonlinearityComponent>", "</GruNonlinearityComponent>")),
                                 ["cycle at node gru1.gru_nonlin_t", "a GruNonlinearityComponent (fast-gru-layer, fast-pgru-layer, fast-norm-pgru-layer)"]),
    "add-log-stddev": ("norm", _swap(("<AddLogStddev> F", "<AddLogStddev> T")),
                       ["cycle at node gru1.s_t_renorm", "a NormalizeComponent with add-log-stddev=true is not supported"]),
    "block-dim": ("norm", _swap(("<NormalizeComponent> <InputDim> 8 ", "<NormalizeComponent> <InputDim> 8 <BlockDim> 4 ")),
                  ["cycle at node gru1.s_t_renorm", "a NormalizeComponent with block-dim is not supported"]),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_cycles_that_are_no_fast_opgru_block_are_refused(built, tmp_path, what):
    """A cycle that holds an OutputGruNonlinearityComponent (or a GruNonlinearityComponent) and is not exactly what fast-opgru-layer /
    fast-norm-opgru-layer emit is refused at load with the node and the reason, in the GRU recogniser's own sentence: gr_text's (or
    the norm variant's) config text with one thing changed."""
    from rhasspy_speech_amd import _lib
    which, edit, needles = REFUSED[what]
    src = built("gr_text")[:2] if which == "basic" else cases.build_case_files(_NORM_TEXT, tmp_path / "src")[:2]
    dst, gd = _edited(src, tmp_path, edit)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    msg = str(ei.value)
    assert "recurrent GRU networks are supported only as fast-opgru-layer / fast-norm-opgru-layer blocks" in msg, msg
    for needle in needles:
        assert needle in msg, (needle, msg)


def _refused(case, root, needle):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = cases.build_case_files(case, root)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert needle in str(ei.value), str(ei.value)


def test_sizes_beyond_the_kernel_s_limits_fail_the_load(tmp_path):
    big = dict(spec=gc._gr((gc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(big, tmp_path / "cell", "recurrent block gru1.gru_nonlin_t: cell dim 2304 is more than the 2048 the HIP kernel takes")
    # (the norm variant: behind the plain one the reference's CollapseModel would fold so wide a W_y into the next layer's affine)
    out = dict(spec=gc._gr((gc._b(cell=32, rec=8, nonrec=4100, norm=True),)), graph="grammar", audio="zeros:0")
    _refused(out, tmp_path / "out", "recurrent block gru1.gru_nonlin_t: output dim 4108 (recurrent + non-recurrent) is more than the 4096 the HIP kernel takes")
    lds = dict(spec=gc._gr((gc._b(cell=2048, rec=512, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(lds, tmp_path / "lds", "recurrent block gru1.gru_nonlin_t: the state and product rows of 16 chains (cell dim 2048 + recurrent dim 512, 197376 bytes) "
                                    "do not fit the 147456 bytes of LDS the HIP kernel keeps them in")


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("gr_basic")[:2]).describe()
    b = _lib.Model(*built("gr_text")[:2]).describe()
    keep = ("op:", "gru:", "nnet:")
    assert [l for l in a.splitlines() if l.startswith(keep)] == [l for l in b.splitlines() if l.startswith(keep)]


# ------------------------------------------------------------------------------------------ the planner under sanitizers

def test_reader_and_planner_under_sanitizers(built, tmp_path):
    """tests/host/gru_plan_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's final.mdl, compiles
    the network, plans every GRU block, builds the weight images and checks their padding is zero; what it prints is what describe()
    says."""
    from rhasspy_speech_amd import _lib, synth
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "gru_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "gru_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "gru_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args, want = [], []
    for name in gc.CASES:
        args += [name, str(_mdl(built(name)[0]))]
        if name in gc.NO_GOLDEN:      # (the dither rule is the engine's, not the reader's: the network itself plans like gr_basic's)
            want += [f"{name} {l}" for l in _gru_lines(name)]
        else:
            text = _lib.Model(*built(name)[:2]).describe()
            want += [f"{name} {l.split()[0]} {l.split()[1]}" if l.startswith("lstm: ") else f"{name} {l}" for l in text.splitlines() if l.startswith(("lstm: ", "gru: "))]
    extra = {
        "x_full_size": (dict(spec=gc._gr((gc._b(cell=1024, rec=256, nonrec=256, norm=True),)), graph="grammar", audio="zeros:0"),
                        "x_full_size gru: gru1.gru_nonlin_t input=32 cell=1024 rec=256 nonrec=256 delay=3 scale=1 norm=1 dropout=0 kernel=gru16x16x4<w8> "
                        "rows_per_block=16 lds=99072 w_zo=32+256 cell_tiles=64 out_tiles=32 grid=chains/16"),
        "x_cell": (dict(spec=gc._gr((gc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0"),
                   "x_cell error: nnet3: recurrent block gru1.gru_nonlin_t: cell dim 2304 is more than the 2048 the HIP kernel takes"),
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

def test_writers_of_the_four_components():
    """Field order as the reference's Write methods have it (nnet-combined-component.cc:2204-2241, nnet-normalize-component.cc:98-111,
    nnet-simple-component.cc:225-236 and 312-319), text form."""
    from rhasspy_speech_amd import synth
    w = synth.KaldiWriter(False)
    synth._w_output_gru_nonlinearity(w, np.array([0.5, -0.25], np.float32))
    assert w.getvalue().decode() == ("<OutputGruNonlinearityComponent> <LearningRate> 0.0010000000474974513 <CellDim> 2 <w_h>  [ 0.5 -0.25 ]\n"
                                     "<ValueAvg>  [ 0.0 0.0 ]\n<DerivAvg>  [ 0.0 0.0 ]\n<SelfRepairTotal> 0.0 <Count> 0.0 <SelfRepairThreshold> 0.20000000298023224 "
                                     "<SelfRepairScale> 9.999999747378752e-06 <Alpha> 4.0 <Rank> 8 <UpdatePeriod> 10 </OutputGruNonlinearityComponent> ")
    w = synth.KaldiWriter(False)
    synth._w_normalize(w, 8)
    assert w.getvalue().decode() == "<NormalizeComponent> <InputDim> 8 <TargetRms> 1.0 <AddLogStddev> F </NormalizeComponent> "
    w = synth.KaldiWriter(False)
    synth._w_dropout(w, 32)
    assert w.getvalue().decode() == "<DropoutComponent> <Dim> 32 <DropoutProportion> 0.0 <DropoutPerFrame> F <TestMode> F </DropoutComponent> "
    w = synth.KaldiWriter(False)
    synth._w_elementwise_product(w, 64, 32)
    assert w.getvalue().decode() == "<ElementwiseProductComponent> <InputDim> 64 <OutputDim> 32 </ElementwiseProductComponent> "
    assert synth.gru_layer_dims(dict(cell=32, rec=8, nonrec=24)) == (32, 8, 24, 32)
    with pytest.raises(ValueError):
        synth.gru_layer_dims(dict(cell=32, rec=8, nonrec=0))
    with pytest.raises(ValueError):
        synth.gru_layer_dims(dict(cell=32, rec=8, nonrec=8, dropout=True))
    assert synth.tiny_spec().gru_layers == ()


def test_block_nodes_are_written_in_xconfig_s_order():
    """The config lines of a block in the order XconfigFastOpgruLayer / XconfigFastNormOpgruLayer emit them (xconfig/gru.py)."""
    from rhasspy_speech_amd import synth

    def names(case):
        spec = cases.case_spec(gc.CASES[case])
        return [l.split("name=")[1].split()[0] for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if " name=gru1." in l]
    assert names("gr_basic") == [f"gru1.{n}" for n in ("z_t_pre", "z_t", "o_t_pre", "o_t", "hpart_t", "gru_nonlin_t", "c_t", "cdoto", "y_t", "s_t_preclip", "s_t")]
    assert names("gr_norm_drop") == [f"gru1.{n}" for n in ("z_t_pre", "z_t_predrop", "z_t", "o_t_pre", "o_t_predrop", "o_t", "hpart_t", "gru_nonlin_t", "c_t", "cdoto",
                                                           "y_t_tmp", "s_t_pre", "s_t_renorm", "s_t", "y_t")]
