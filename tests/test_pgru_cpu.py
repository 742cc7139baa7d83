"""TDNN-PGRU / TDNN-GRU models (recurrent blocks around a GruNonlinearityComponent: fast-pgru-layer / fast-norm-pgru-layer /
fast-gru-layer) without a GPU: the goldens of tests/pgru_cases.py, the float64 restatement against them, the block recogniser and
its refusals, the set-up's restatement (contexts, collapsed network, the dither rule), the load-time planner through a stand-alone
host program under the address and undefined-behaviour sanitizers, and the synthetic model writer."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import cases
from tests import gru_cases as gc
from tests import pgru_cases as pc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in pc.CASES if n not in pc.NO_GOLDEN]
DECODED = [n for n in WITH_GOLDEN if n != "pg_len0"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = pc.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _mdl(model_dir):
    return model_dir / "model" / "model" / "final.mdl"


# ------------------------------------------------------------------------------------------ goldens

def test_goldens_are_there_for_every_case():
    for name in WITH_GOLDEN:
        g = pc.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(pc.CASES[name], sort_keys=True), name      # (made from this table)
        if name == "pg_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "context", "collapsed"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                    for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "pg_stack":
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        spec = cases.case_spec(pc.CASES[name])
        assert g["input"].shape[1] == spec.feat_dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape
        fsf = pc.fsf_of(name)
        assert int(g["offline_num_frames"]) == (g["input"].shape[0] + fsf - 1) // fsf
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
    frames = {n: pc.load_golden(n)["input"].shape[0] for n in pc.LENGTHS[1:]}
    assert frames == {"pg_len1": 1, "pg_len2": 2, "pg_len25": 25, "pg_len47": 47}      # (the chunk is 24 frames)
    assert sorted(p.stem for p in pc.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in pc.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


@pytest.mark.parametrize("name", DECODED)
def test_nbest_hypotheses_are_far_enough_apart(name):
    """Adjacent n-best hypotheses differ in total cost by more than 0.02, ten times the 2e-3 cost tolerance of the GPU tests: the order
    of the list is not a matter of rounding.  A condition on the reference's output alone (the audio seeds were chosen for it)."""
    g = pc.load_golden(name)
    for mode in ("offline", "stream"):
        total = g[f"{mode}_graph_cost"].astype(np.float64) + g[f"{mode}_acoustic_cost"]
        if len(total) > 1:
            assert np.diff(total).min() > 0.02, (name, mode, np.diff(total).min())


@pytest.mark.parametrize("name", DECODED)
def test_float64_restatement_agrees_with_the_reference(name):
    """pgru_cases.Float64Net -- GruNonlinearityComponent::Propagate over the golden `input` rows between the sigmoids, W_y,
    NormalizePerRow and the truncation scale (without a projection: the scaled cell as the state), chains started where the block's
    feed-forward input first exists -- against the reference's offline_loglikes, within 2.5e-5: a quarter of the device bound (the
    bound of test_gru_cpu.py).  Measured when the goldens were made: 2.4e-07 (pg_len2) to 4.7e-06 (pg_norm); pg_stack 2.9e-06,
    pg_norm_drop 2.2e-06, every other case below 8.5e-07."""
    g = pc.load_golden(name)
    ll, blocks = pc.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(blocks) == len(pc.block_dims(name))
    for rows, (_kind, _k, _in, out_dim, _layer) in zip(blocks, pc.block_dims(name)):
        assert rows.shape == (g["input"].shape[0], out_dim)
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}")
    assert diff < 2.5e-5, diff
    if "offline_ivector" not in g.files:      # (without an extractor the streamed rows are the offline ones)
        np.testing.assert_array_equal(g["stream_loglikes"], g["offline_loglikes"])


# ------------------------------------------------------------------------------------------ load and describe

def _pgru_lines(name):
    """The `pgru:` lines of the case by the planner's rules: k extents rounded up to 16, LDS pitches of k + 4 floats, two tiles of s
    rows and one of r . s rows (recurrent dim wide; the cell dim without a projection) and, with a projection, one of c rows for 16
    chains."""
    out = []
    for kind, k, in_dim, _out, layer in pc.block_dims(name):
        if kind != "pgru":
            continue
        cell, rec, nonrec = int(layer["cell"]), int(layer["rec"]), int(layer["nonrec"])
        R = rec if rec > 0 else cell
        k_s, k_c = (R + 15) // 16 * 16, (cell + 15) // 16 * 16
        lds = 16 * 4 * (3 * (k_s + 4) + ((k_c + 4) if rec > 0 else 0))
        out.append(f"pgru: pgru{k}.gru_nonlin_t input={in_dim} cell={cell} rec={rec} nonrec={nonrec} delay={int(layer.get('delay', 3))} "
                   f"scale={float(layer.get('scale', 1.0)):g} norm={int(bool(layer.get('norm', False)))} dropout={int(bool(layer.get('dropout', False)))} "
                   f"kernel=pgru16x16x4<w8> rows_per_block=16 lds={lds} w_zr={in_dim}+{R} cell_tiles={k_c // 16} rec_tiles={k_s // 16} "
                   f"out_tiles={(rec + nonrec + 15) // 16} grid=chains/16")
    return out


_NONLIN = {"lstm": "lstm_nonlin", "gru": "gru_nonlin_t", "pgru": "gru_nonlin_t"}


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_blocks(built, name):
    """The parent refused these directories at load ("a GruNonlinearityComponent ...: its h needs a third serial matrix product, which
    the HIP kernel does not have").  Now they load on the host: per block ONE layer GEMM over the feed-forward columns of W_z, W_r
    and W_hpart (cell + R + cell rows), an `op: pgru` and a `pgru:` line with the case's dims and what the planner chose; the context
    is the reference's."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    assert [l for l in text.splitlines() if l.startswith("pgru: ")] == _pgru_lines(name)
    ops = [l for l in text.splitlines() if l.startswith("op: ")]
    rec_ops = [l for l in ops if l.startswith(("op: lstm ", "op: gru ", "op: pgru "))]
    dims = pc.block_dims(name)
    assert [l.split()[1:3] for l in rec_ops] == [[kind, f"{kind}{k}.{_NONLIN[kind]}"] for kind, k, *_r in dims]
    for kind, k, in_dim, _out, layer in dims:
        if kind != "pgru":
            continue
        cell, rec = int(layer["cell"]), int(layer["rec"])
        R = rec if rec > 0 else cell
        at = [i for i, l in enumerate(ops) if l.startswith(f"op: pgru pgru{k}.gru_nonlin_t out_dim={2 * cell} terms=1 stages=0")]
        assert len(at) == 1 and ops[at[0] - 1].startswith(f"op: gemm pgru{k}.gru_nonlin_t.x out_dim={2 * cell + R} k={in_dim} "), ops
        if layer.get("norm", False):     # BatchNorm on y: an elementwise op of its own, the block's rows stay as the block wrote them
            assert f"op: eltwise pgru{k}.y_t out_dim={rec + int(layer['nonrec'])} terms=1 stages=1" in "\n".join(ops)
    fsf = pc.fsf_of(name)
    if name == "pg_fsf3":        # delay 3 under factor 3 and offsets {-3, 0, 3} above: one residue class
        assert all(l.endswith(" rows=every-3") for l in rec_ops)
    else:                        # (pg_fsf3_d2: delay 2 visits every class; the layers above it still run on every third row)
        assert not any("rows=every" in l for l in rec_ops)
        assert ("rows=every-3" in text) == (fsf == 3)
    left, right = pc.contexts(name)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]
    if name != "pg_len0":
        assert [left, right] == pc.load_golden(name)["context"].tolist()      # (what the reference's looped decodable computed)


def test_an_opgru_model_describes_no_pgru_block(tmp_path):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = gc.build_case_files("gr_basic", tmp_path)
    text = _lib.Model(md, gd).describe()
    assert "pgru" not in text and text.count("\ngru: ") == 1 and text.count("\nop: gru ") == 1


def _setup(md, fsf):
    from rhasspy_speech_amd import _lib
    lib = _lib.load_library()
    lib.rs_nnet3_setup_subsampled.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    n, cert, buf = C.c_int64(), C.c_int32(), C.create_string_buffer(1 << 16)
    assert lib.rs_nnet3_setup_subsampled(str(_mdl(md)).encode(), 24, fsf, C.byref(n), C.byref(cert), buf, len(buf)) == 0
    return n.value, cert.value, buf.value.decode().splitlines()


@pytest.mark.parametrize("name", DECODED)
def test_setup_leaves_the_reference_s_network(built, name):
    """rs_nnet3_setup on a network with such blocks: the collapsed network is the one rs-dump printed after the reference's
    CollapseModel.  Of a block nothing collapses -- its lines are those synth.py wrote; the norm variant's BatchNorm stays a node of
    its own behind W_y -- and the rand() position is reported as not certain."""
    from rhasspy_speech_amd import synth
    _, certain, lines = _setup(built(name)[0], pc.fsf_of(name))
    assert certain == 0
    assert lines == bytes(pc.load_golden(name)["collapsed"]).decode().splitlines()
    spec = cases.case_spec(pc.CASES[name])
    written = [l for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if " name=pgru" in l]
    assert len(written) >= 8 and [l for l in lines if " name=pgru" in l] == written      # (a fast-gru-layer block has eight nodes)
    if any(layer.get("norm", False) for layer in spec.pgru_layers):
        assert any(".y_t component=" in l and ".batchnorm input=" in l and l.endswith(".y_t_tmp") for l in lines)


def test_default_dither_is_refused_with_the_recurrence_named(built):
    """pg_dither_default: the reference's set-up accepts the model (gen_pgru_golden.py runs it); the rand() calls of a recurrent
    compilation are not replayed, so by the existing rule the model loads with --dither=0 only."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("pg_dither_default")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    msg = str(ei.value)
    assert "--dither=1" in msg and "cannot be derived for this network" in msg and "the network is recurrent (a cycle through node pgru1." in msg, msg


# ------------------------------------------------------------------------------------------ refusals

_NORM_TEXT = dict(spec=pc._pg((pc._b(norm=True),), binary=False), graph="grammar", audio="zeros:0")


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


_S3, _C3 = "IfDefined(Offset(pgru1.s_t, -3))", "IfDefined(Offset(pgru1.c_t, -3))"
_ZPRE = "component-node name=pgru1.z_t_pre component=pgru1.W_z.xs input=Append(tdnn2.batchnorm, " + _S3 + ")"
_RPRE = "component-node name=pgru1.r_t_pre component=pgru1.W_r.xs input=Append(tdnn2.batchnorm, " + _S3 + ")"
_NL_IN = "input=Append(pgru1.z_t, pgru1.r_t, pgru1.hpart_t, " + _C3 + ", " + _S3 + ")"
_WHAT = "a GruNonlinearityComponent (fast-gru-layer, fast-pgru-layer, fast-norm-pgru-layer) "

REFUSED = {
    "a positive delay": ("basic", _swap((_C3, "IfDefined(Offset(pgru1.c_t, 3))")),
                         ["cycle at node pgru1.gru_nonlin_t", "a positive delay, Offset(pgru1.c_t, 3)"]),
    "different delays": ("basic", _swap((_ZPRE, _ZPRE.replace("-3", "-2"))),
                         ["cycle at node pgru1.z_t_pre", "two different delays in one block, 2 and 3"]),
    "different delays of c and s": ("basic", _swap((_NL_IN, _NL_IN.replace(_C3, _C3.replace("-3", "-2")))),
                                    ["cycle at node pgru1.gru_nonlin_t", "two different delays in one block, 3 and 2"]),
    "a delay outside 1..8": ("basic", lambda t: _swap((_C3, _C3.replace("-3", "-9")))(_swap((_S3, _S3.replace("-3", "-9")), count=3)(t)),
                             ["cycle at node pgru1.gru_nonlin_t", "a delay of 9 frames; the HIP kernel takes 1 to 8"]),
    "a state not inside IfDefined": ("basic", _swap((_C3, "Offset(pgru1.c_t, -3)")),
                                     ["cycle at node pgru1.gru_nonlin_t", "its recurrent input pgru1.c_t is not inside IfDefined()"]),
    "W_r of the wrong rows": ("basic", _swap((_RPRE, _RPRE.replace("component=pgru1.W_r.xs", "component=pgru1.W_z.xs"))),
                              ["cycle at node pgru1.r_t_pre", "the gate's affine has 32 rows, not the recurrent dim 8"]),
    "<w_h> of the wrong shape": ("basic", _swap(("<CellDim> 32 <RecurrentDim> 8 ", "<CellDim> 32 <RecurrentDim> 4 ")),
                                 ["cycle at node pgru1.gru_nonlin_t", _WHAT + "whose <w_h> is 32 x 8, not cell-dim 32 x recurrent-dim 4"]),
    "no <RecurrentDim>": ("basic", _swap(("<CellDim> 32 <RecurrentDim> 8 ", "<CellDim> 32 ")),
                          ["cycle at node pgru1.gru_nonlin_t", _WHAT + "without a <RecurrentDim>, over an input of 5 parts"]),
    "a projected component over a four-part input": ("basic", _swap((_NL_IN, _NL_IN.replace(_C3 + ", ", ""))),
                                                     ["cycle at node pgru1.gru_nonlin_t", _WHAT + "with <RecurrentDim> 8 and <CellDim> 32 over a four-part input"]),
    "different feed-forward inputs": ("basic", _swap((_RPRE, _RPRE.replace("Append(tdnn2.batchnorm,", "Append(Scale(0.5, tdnn2.batchnorm),"))),
                                      ["cycle at node pgru1.r_t_pre", "the two gates do not read the same feed-forward input"]),
    "a second nonlinearity": ("basic", _add_nodes(["component-node name=pgru1.nl2 component=pgru1.gru_nonlin " + _NL_IN,
                                                   "dim-range-node name=pgru1.c2 input-node=pgru1.nl2 dim-offset=32 dim=32"],
                                                  ("component=pgru1.W_y.c input=pgru1.c_t", "component=pgru1.W_y.c input=Sum(pgru1.c_t, pgru1.c2)")),
                              ["cycle at node pgru1.", "a second GruNonlinearityComponent in one cycle"]),
    "a node of the cycle outside the block": ("basic", _add_nodes(["component-node name=pgru1.extra component=pgru1.z input=pgru1.z_t_pre"],
                                                                   ("component=pgru1.W_y.c input=pgru1.c_t", "component=pgru1.W_y.c input=Sum(pgru1.c_t, pgru1.extra)")),
                                              ["cycle at node pgru1.y_t", "W_y's input is not the cell state pgru1.c_t"]),
    "add-log-stddev": ("norm", _swap(("<AddLogStddev> F", "<AddLogStddev> T")),
                       ["cycle at node pgru1.s_t_renorm", "a NormalizeComponent with add-log-stddev=true is not supported"]),
    "block-dim": ("norm", _swap(("<NormalizeComponent> <InputDim> 8 ", "<NormalizeComponent> <InputDim> 8 <BlockDim> 4 ")),
                  ["cycle at node pgru1.s_t_renorm", "a NormalizeComponent with block-dim is not supported"]),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_cycles_that_are_no_fast_pgru_block_are_refused(built, tmp_path, what):
    """A cycle that holds a GruNonlinearityComponent and is not exactly what fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer
    emit is refused at load with the node and the reason, in the GRU recogniser's sentence extended by the three layers: pg_text's
    (or the norm variant's) config text with one thing changed."""
    from rhasspy_speech_amd import _lib
    which, edit, needles = REFUSED[what]
    src = built("pg_text")[:2] if which == "basic" else cases.build_case_files(_NORM_TEXT, tmp_path / "src")[:2]
    dst, gd = _edited(src, tmp_path, edit)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    msg = str(ei.value)
    assert ("recurrent GRU networks are supported only as fast-opgru-layer / fast-norm-opgru-layer blocks and, around a GruNonlinearityComponent, as "
            "fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer blocks") in msg, msg
    for needle in needles:
        assert needle in msg, (needle, msg)


def _refused(case, root, needle):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = cases.build_case_files(case, root)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert needle in str(ei.value), str(ei.value)


def test_sizes_beyond_the_kernel_s_limits_fail_the_load(tmp_path):
    from rhasspy_speech_amd import _lib
    big = dict(spec=pc._pg((pc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(big, tmp_path / "cell", "recurrent block pgru1.gru_nonlin_t: cell dim 2304 is more than the 2048 the HIP kernel takes")
    out = dict(spec=pc._pg((pc._b(cell=32, rec=8, nonrec=4100, norm=True),)), graph="grammar", audio="zeros:0")
    _refused(out, tmp_path / "out", "recurrent block pgru1.gru_nonlin_t: output dim 4108 (recurrent + non-recurrent) is more than the 4096 the HIP kernel takes")
    # 64 bytes x (three tiles of 512 + 4 and one of 2048 + 4 floats)
    lds = dict(spec=pc._pg((pc._b(cell=2048, rec=512, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(lds, tmp_path / "lds", "recurrent block pgru1.gru_nonlin_t: the state, product and cell rows of 16 chains (cell dim 2048, recurrent dim 512, 230400 bytes) "
                                    "do not fit the 147456 bytes of LDS the HIP kernel keeps them in")
    # fast-gru-layer: three tiles of cell + 4 floats; 752 is the widest cell that fits, 768 does not
    plain = dict(spec=pc._pg((pc._plain(cell=768),)), graph="grammar", audio="zeros:0")
    _refused(plain, tmp_path / "plain", "recurrent block pgru1.gru_nonlin_t: the state, product and cell rows of 16 chains (cell dim 768, recurrent dim 768, 148224 bytes) "
                                        "do not fit the 147456 bytes of LDS the HIP kernel keeps them in")
    fits = dict(spec=pc._pg((pc._plain(cell=752),)), graph="grammar", audio="zeros:0")
    md, gd, _, _ = cases.build_case_files(fits, tmp_path / "fits")
    assert " cell=752 rec=0 nonrec=0 " in _lib.Model(md, gd).describe() and 64 * 3 * 756 == 145152 <= 147456


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("pg_basic")[:2]).describe()
    b = _lib.Model(*built("pg_text")[:2]).describe()
    keep = ("op:", "pgru:", "nnet:")
    assert [l for l in a.splitlines() if l.startswith(keep)] == [l for l in b.splitlines() if l.startswith(keep)]


# ------------------------------------------------------------------------------------------ the planner under sanitizers

def test_reader_and_planner_under_sanitizers(built, tmp_path):
    """tests/host/pgru_plan_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's final.mdl, compiles
    the network, plans every block around a GruNonlinearityComponent, builds the weight images and checks their padding is zero;
    what it prints is what describe() says.  A recipe-size block in both variants plans inside the kernel's 144 KiB of LDS."""
    from rhasspy_speech_amd import _lib, synth
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "pgru_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "pgru_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "pgru_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args, want = [], []
    for name in pc.CASES:
        args += [name, str(_mdl(built(name)[0]))]
        if name in pc.NO_GOLDEN:      # (the dither rule is the engine's, not the reader's: the network itself plans like pg_basic's)
            want += [f"{name} {l}" for l in _pgru_lines(name)]
        else:
            text = _lib.Model(*built(name)[:2]).describe()
            want += [f"{name} {l.split()[0]} {l.split()[1]}" if l.startswith(("lstm: ", "gru: ")) else f"{name} {l}" for l in text.splitlines()
                     if l.startswith(("lstm: ", "gru: ", "pgru: "))]
    full = "input=32 cell=1024 rec=256 nonrec=256 delay=3 scale=1 norm={n} dropout=0 kernel=pgru16x16x4<w8> rows_per_block=16 lds=115712 w_zr=32+256 " \
           "cell_tiles=64 rec_tiles=16 out_tiles=32 grid=chains/16"
    assert 64 * (3 * 260 + 1028) == 115712 <= 144 * 1024
    extra = {
        "x_full_size": (dict(spec=pc._pg((pc._b(cell=1024, rec=256, nonrec=256),)), graph="grammar", audio="zeros:0"),
                        "x_full_size pgru: pgru1.gru_nonlin_t " + full.format(n=0)),
        "x_full_size_norm": (dict(spec=pc._pg((pc._b(cell=1024, rec=256, nonrec=256, norm=True),)), graph="grammar", audio="zeros:0"),
                             "x_full_size_norm pgru: pgru1.gru_nonlin_t " + full.format(n=1)),
        "x_plain_512": (dict(spec=pc._pg((pc._plain(cell=512),)), graph="grammar", audio="zeros:0"),
                        "x_plain_512 pgru: pgru1.gru_nonlin_t input=32 cell=512 rec=0 nonrec=0 delay=3 scale=1 norm=0 dropout=0 kernel=pgru16x16x4<w8> "
                        "rows_per_block=16 lds=99072 w_zr=32+512 cell_tiles=32 rec_tiles=32 out_tiles=0 grid=chains/16"),
        "x_cell": (dict(spec=pc._pg((pc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0"),
                   "x_cell error: nnet3: recurrent block pgru1.gru_nonlin_t: cell dim 2304 is more than the 2048 the HIP kernel takes"),
        "x_none": (dict(spec=dict(), graph="grammar", audio="zeros:0"), "x_none no recurrent block"),
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

def test_writer_of_the_component():
    """Field order as GruNonlinearityComponent::Write has it (nnet-combined-component.cc:1726-1767), text form: <RecurrentDim> behind
    <CellDim>, <w_h> a cell x recurrent matrix, <RankInOut> with its two integers."""
    from rhasspy_speech_amd import synth
    w = synth.KaldiWriter(False)
    synth._w_gru_nonlinearity(w, np.array([[0.5, -0.25, 1.0], [2.0, 0.0, -1.0]], np.float32))
    assert w.getvalue().decode() == ("<GruNonlinearityComponent> <LearningRate> 0.0010000000474974513 <CellDim> 2 <RecurrentDim> 3 <w_h>  [\n  0.5 -0.25 1.0\n"
                                     "  2.0 0.0 -1.0 ]\n<ValueAvg>  [ 0.0 0.0 ]\n<DerivAvg>  [ 0.0 0.0 ]\n<SelfRepairTotal> 0.0 <Count> 0.0 <SelfRepairThreshold> "
                                     "0.20000000298023224 <SelfRepairScale> 9.999999747378752e-06 <Alpha> 4.0 <RankInOut> 8 8 <UpdatePeriod> 10 "
                                     "</GruNonlinearityComponent> ")
    assert synth.pgru_layer_dims(dict(cell=32, rec=8, nonrec=24)) == (32, 8, 24, 32)
    assert synth.pgru_layer_dims(dict(cell=32, rec=0, nonrec=0)) == (32, 32, 0, 32)
    for bad in (dict(cell=32, rec=8, nonrec=0), dict(cell=32, rec=0, nonrec=8), dict(cell=32, rec=8, nonrec=8, dropout=True), dict(cell=32, rec=0, nonrec=0, norm=True)):
        with pytest.raises(ValueError):
            synth.pgru_layer_dims(bad)
    assert synth.tiny_spec().pgru_layers == ()


def test_block_nodes_are_written_in_xconfig_s_order():
    """The config lines of a block in the order XconfigFastPgruLayer / XconfigFastNormPgruLayer / XconfigFastGruLayer emit them
    (xconfig/gru.py), and the components' names."""
    from rhasspy_speech_amd import synth

    def names(case, what=" name=pgru1."):
        spec = cases.case_spec(pc.CASES[case])
        return [l.split("name=")[1].split()[0] for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if what in l]
    assert names("pg_basic") == [f"pgru1.{n}" for n in ("z_t_pre", "z_t", "r_t_pre", "r_t", "hpart_t", "gru_nonlin_t", "c_t", "y_t", "s_t_pre", "s_t")]
    assert names("pg_plain") == [f"pgru1.{n}" for n in ("z_t_pre", "z_t", "r_t_pre", "r_t", "hpart_t", "gru_nonlin_t", "y_t", "s_t")]
    assert names("pg_norm_drop") == [f"pgru1.{n}" for n in ("z_t_pre", "z_t_predrop", "z_t", "r_t_pre", "r_t_predrop", "r_t", "hpart_t", "gru_nonlin_t", "c_t",
                                                            "y_t_tmp", "s_t_pre", "s_t_renorm", "s_t", "y_t")]

    def comps(case):
        spec = cases.case_spec(pc.CASES[case])
        return [n for n, _ in synth.build_nnet(spec, np.random.default_rng(spec.seed))[1] if n.startswith("pgru1.")]
    assert comps("pg_plain") == [f"pgru1.{n}" for n in ("W_z.xh", "W_r.xh", "W_hpart.x", "z", "r", "gru_nonlin", "s_r")]
    assert comps("pg_norm_drop") == [f"pgru1.{n}" for n in ("W_z.xs", "W_r.xs", "W_hpart.x", "z", "r", "dropout_z", "dropout_r", "gru_nonlin", "W_y.c", "renorm", "s_r",
                                                            "batchnorm")]
