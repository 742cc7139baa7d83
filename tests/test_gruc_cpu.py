"""TDNN-GRU models whose cell is spelled out as separate components (gru-layer / pgru-layer / norm-pgru-layer / opgru-layer /
norm-opgru-layer) without a GPU: the goldens of tests/gruc_cases.py, the float64 restatement against them, the block recogniser and
its refusals, the set-up's restatement (contexts, collapsed network, the dither rule), the reader, recogniser and planners through a
stand-alone host program under the address and undefined-behaviour sanitizers, and the synthetic model writer."""
import ctypes as C
import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import cases
from tests import gru_cases as grc
from tests import gruc_cases as gc
from tests import pgru_cases as pc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
WITH_GOLDEN = [n for n in gc.CASES if n not in gc.NO_GOLDEN]
DECODED = [n for n in WITH_GOLDEN if n != "gc_len0"]
FIVE = "one gru-layer / pgru-layer / norm-pgru-layer / opgru-layer / norm-opgru-layer block"


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
        if name == "gc_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "context", "collapsed"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                    for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if name == "gc_stack":
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
    assert frames == {"gc_len1": 1, "gc_len2": 2, "gc_len25": 25, "gc_len47": 47}      # (the chunk is 24 frames)
    assert sorted(p.stem for p in gc.GOLDEN.iterdir()) == sorted(WITH_GOLDEN)
    for p in gc.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stat().st_size < (1 << 20)


def test_the_case_table_covers_the_five_layers_and_both_kernels_edges():
    """Each of the five layers at cell 32 / R 8 / P 8 / delay 3, one odd and one wide shape per family, gru-layer wide, both norm forms
    with dropout components: a condition on the table, so that a later edit cannot quietly drop a layer."""
    def layers(name):
        s = gc.CASES[name]["spec"]
        return [("pgru", l) for l in s["pgru_layers"] if gc.is_composed(l)] + [("gru", l) for l in s["gru_layers"] if gc.is_composed(l)]
    seen = set()
    for name in WITH_GOLDEN:
        for fam, l in layers(name):
            seen.add((fam, l["rec"] > 0, bool(l.get("norm")), bool(l.get("dropout")), l["cell"], l["delay"]))
    for want in (("pgru", False, False, False, 32, 3), ("pgru", True, False, False, 32, 3), ("pgru", True, True, False, 32, 3), ("gru", True, False, False, 32, 3),
                 ("gru", True, True, False, 32, 3), ("pgru", True, True, True, 32, 3), ("gru", True, True, True, 32, 3), ("pgru", True, False, False, 20, 1),
                 ("gru", True, False, False, 20, 1), ("pgru", True, False, False, 160, 3), ("gru", True, False, False, 160, 3), ("pgru", False, False, False, 144, 3),
                 ("gru", True, False, False, 32, 8), ("gru", True, False, False, 32, 2)):
        assert want in seen, want


@pytest.mark.parametrize("name", DECODED)
def test_nbest_hypotheses_are_far_enough_apart(name):
    """Adjacent n-best hypotheses differ in total cost by more than 0.02, ten times the 2e-3 cost tolerance of the GPU tests (the bound
    of test_pgru_cpu.py): the order of the list is not a matter of rounding.  A condition on the reference's output alone (the audio
    seeds were chosen for it)."""
    g = gc.load_golden(name)
    for mode in ("offline", "stream"):
        total = g[f"{mode}_graph_cost"].astype(np.float64) + g[f"{mode}_acoustic_cost"]
        if len(total) > 1:
            assert np.diff(total).min() > 0.02, (name, mode, np.diff(total).min())


@pytest.mark.parametrize("name", DECODED)
def test_float64_restatement_agrees_with_the_reference(name):
    """gruc_cases.Float64Net -- the composed cell node by node over the golden `input` rows, y = h (1 - z) + y[t - d] z with the
    descriptor's Scale and Const read from the config, chains started where the block's feed-forward input first exists -- against
    the reference's offline_loglikes, within the project's 1e-4.  Measured when the goldens were made: 2.5e-07 (gc_opgru) to 2.5e-06
    (gc_npgru_drop); the norm forms 9.7e-07 to 2.5e-06, every other case below 8.9e-07."""
    g = gc.load_golden(name)
    ll, blocks = gc.restate(name, g)
    assert ll.shape == g["offline_loglikes"].shape and len(blocks) == len(gc.block_dims(name))
    for rows, (_kind, _k, _in, out_dim, _layer) in zip(blocks, gc.block_dims(name)):
        assert rows.shape == (g["input"].shape[0], out_dim)
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: max |restatement - reference| {diff:.4g}")
    assert diff < 1e-4, diff
    if "offline_ivector" not in g.files:      # (without an extractor the streamed rows are the offline ones)
        np.testing.assert_array_equal(g["stream_loglikes"], g["offline_loglikes"])


# ------------------------------------------------------------------------------------------ load and describe

def _block_name(kind, k, layer):
    if kind == "lstm":
        return f"lstm{k}.lstm_nonlin"
    return f"{kind}{k}.y_t" if gc.is_composed(layer) else f"{kind}{k}.gru_nonlin_t"


def _block_lines(name, want_kind):
    """The `gru:` / `pgru:` lines of the case by the planners' rules (k extents rounded up to 16, LDS pitches of k + 4 floats, 16
    chains): a composed block's line is its family's, named after y_t, with the composed kernel and ` form=composed` at its end."""
    out = []
    for kind, k, in_dim, _out, layer in gc.block_dims(name):
        if kind != want_kind:
            continue
        cell, rec, nonrec = int(layer["cell"]), int(layer["rec"]), int(layer["nonrec"])
        comp = gc.is_composed(layer)
        R = rec if rec > 0 else cell
        k_s, k_c = (R + 15) // 16 * 16, (cell + 15) // 16 * 16
        head = (f"{kind}: {_block_name(kind, k, layer)} input={in_dim} cell={cell} rec={rec} nonrec={nonrec} delay={int(layer.get('delay', 3))} "
                f"scale={float(layer.get('scale', 1.0)):g} norm={int(bool(layer.get('norm', False)))} dropout={int(bool(layer.get('dropout', False)))} ")
        if kind == "pgru":
            lds = 16 * 4 * (3 * (k_s + 4) + ((k_c + 4) if rec > 0 else 0))
            line = head + (f"kernel={'pgruc' if comp else 'pgru'}16x16x4<w8> rows_per_block=16 lds={lds} w_zr={in_dim}+{R} cell_tiles={k_c // 16} "
                           f"rec_tiles={k_s // 16} out_tiles={(rec + nonrec + 15) // 16} grid=chains/16")
        else:
            lds = 16 * 4 * (2 * (k_s + 4) + k_c + 4)
            line = head + (f"kernel={'gruc' if comp else 'gru'}16x16x4<w8> rows_per_block=16 lds={lds} w_zo={in_dim}+{R} cell_tiles={k_c // 16} "
                           f"out_tiles={(rec + nonrec + 15) // 16} grid=chains/16")
        out.append(line + (" form=composed" if comp else ""))
    return out


@pytest.mark.parametrize("name", WITH_GOLDEN)
def test_model_loads_and_describes_its_blocks(built, name):
    """The parent refused these directories at load ("... the non-fast GRU layers are not supported ...").  Now they load on the host:
    per block ONE layer GEMM over the feed-forward columns of the three affines (cell + R + cell rows; 3 cell for the output-gate
    family, whose W_h.UW has no recurrent columns), an `op: pgru` / `op: gru` and a `pgru:` / `gru:` line with the case's dims, what
    the planner chose and the composed mark; the context is the reference's."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    text = _lib.Model(md, gd).describe()
    assert [l for l in text.splitlines() if l.startswith("pgru: ")] == _block_lines(name, "pgru")
    assert [l for l in text.splitlines() if l.startswith("gru: ")] == _block_lines(name, "gru")
    ops = [l for l in text.splitlines() if l.startswith("op: ")]
    rec_ops = [l for l in ops if l.startswith(("op: lstm ", "op: gru ", "op: pgru "))]
    dims = gc.block_dims(name)
    assert [l.split()[1:3] for l in rec_ops] == [[kind, _block_name(kind, k, layer)] for kind, k, _i, _o, layer in dims]
    for kind, k, in_dim, _out, layer in dims:
        if kind == "lstm":
            continue
        cell, rec = int(layer["cell"]), int(layer["rec"])
        R = rec if rec > 0 else cell
        bname = _block_name(kind, k, layer)
        at = [i for i, l in enumerate(ops) if l.startswith(f"op: {kind} {bname} out_dim={2 * cell} terms=1 stages=0")]
        pre = 2 * cell + R if kind == "pgru" else 3 * cell
        assert len(at) == 1 and ops[at[0] - 1].startswith(f"op: gemm {bname}.x out_dim={pre} k={in_dim} "), ops
        if layer.get("norm", False) and gc.is_composed(layer):     # BatchNorm on sn: an elementwise op of its own, the block's rows stay as the block wrote them
            assert f"op: eltwise {kind}{k}.sn_t out_dim={rec + int(layer['nonrec'])} terms=1 stages=1" in "\n".join(ops)
    fsf = gc.fsf_of(name)
    if name == "gc_fsf3":        # delay 3 under factor 3 and offsets {-3, 0, 3} above: one residue class
        assert all(l.endswith(" rows=every-3") for l in rec_ops)
    else:                        # (gc_fsf3_d2: delay 2 visits every class; the layers above it still run on every third row)
        assert not any("rows=every" in l for l in rec_ops)
        assert ("rows=every-3" in text) == (fsf == 3)
    left, right = gc.contexts(name)
    assert f" left_context={left} right_context={right} " in text, text.splitlines()[3]
    if name != "gc_len0":
        assert [left, right] == gc.load_golden(name)["context"].tolist()      # (what the reference's looped decodable computed)


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
    CollapseModel.  Of a composed block nothing collapses -- its lines are those synth.py wrote, the dropout nodes included; the norm
    forms' BatchNorm stays a node of its own behind W_s.ys, which the dim-range reads too -- and the rand() position is reported as
    not certain."""
    from rhasspy_speech_amd import synth
    _, certain, lines = _setup(built(name)[0], gc.fsf_of(name))
    assert certain == 0
    assert lines == bytes(gc.load_golden(name)["collapsed"]).decode().splitlines()
    spec = cases.case_spec(gc.CASES[name])
    for kind, k, _i, _o, layer in gc.block_dims(name):
        if kind == "lstm" or not gc.is_composed(layer):
            continue
        tag = f" name={kind}{k}."
        written = [l for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if tag in l]
        assert len(written) >= 11 and [l for l in lines if tag in l] == written      # (a gru-layer block has eleven nodes)
        if layer.get("norm", False):
            assert any(f"{kind}{k}.sn_t component=" in l and ".batchnorm input=" in l and l.endswith(".sn_nobatchnorm_t") for l in lines)


def test_default_dither_is_refused_with_the_recurrence_named(built):
    """gc_dither_default: the reference's set-up accepts the model (gen_gruc_golden.py runs it); the rand() calls of a recurrent
    compilation are not replayed, so by the existing rule the model loads with --dither=0 only."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built("gc_dither_default")
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    msg = str(ei.value)
    assert "--dither=1" in msg and "cannot be derived for this network" in msg and "the network is recurrent (a cycle through node pgru1." in msg, msg


# ------------------------------------------------------------------------------------------ refusals

_ONORM_TEXT = dict(spec=gc._net(gru=(gc._b(norm=True, dropout=True),), binary=False), graph="grammar", audio="zeros:0")
_PLAIN_TEXT = dict(spec=gc._net((gc._plain(),), binary=False), graph="grammar", audio="zeros:0")


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


_S3, _Y3 = "IfDefined(Offset(pgru1.s_t, -3))", "IfDefined(Offset(pgru1.y_t, -3))"
_RPRE = "component-node name=pgru1.r_t_pre component=pgru1.W_z.xs_r input=Append(tdnn2.batchnorm, " + _S3 + ")"
_Y2 = "input=Append(" + _Y3 + ", pgru1.z_t)"
_TDNN3 = "input=Append(Offset(pgru1.sn_t, -3), pgru1.sn_t, Offset(pgru1.sn_t, 3))"

REFUSED = {
    "another Const value": ("basic", _swap(("Const(1, 32)", "Const(0.5, 32)")),
                            ["cycle at node pgru1.y1_t", "its second input adds Const(0.500000), not Const(1.0): it is not 1 - z_t"]),
    "another Scale": ("basic", _swap(("Scale(-1, pgru1.z_t)", "Scale(-0.5, pgru1.z_t)")),
                      ["cycle at node pgru1.y1_t", "its second input scales pgru1.z_t by -0.500000, not by -1.0: it is not 1 - z_t"]),
    "Const and Scale the other way round": ("basic", _swap(("Sum(Scale(-1, pgru1.z_t), Const(1, 32))", "Sum(Const(1, 32), Scale(-1, pgru1.z_t))")),
                                            ["cycle at node pgru1.y1_t", "its second input is not Sum(Scale(-1.0, z_t), Const(1.0, cell-dim)), in that order"]),
    "two delays": ("basic", _swap((_Y3, _Y3.replace("-3", "-2"))),
                   ["cycle at node pgru1.z_t_pre", "two different delays in one block, 3 and 2"]),
    "a positive delay": ("basic", _swap((_Y3, "IfDefined(Offset(pgru1.y_t, 3))")),
                         ["cycle at node pgru1.y2_t", "a positive delay, Offset(pgru1.y_t, 3)"]),
    "delay 9": ("basic", lambda t: _swap((_Y3, _Y3.replace("-3", "-9")))(_swap((_S3, _S3.replace("-3", "-9")), count=3)(t)),
                ["cycle at node pgru1.y2_t", "a delay of 9 frames; the HIP kernel takes 1 to 8"]),
    "a state not inside IfDefined": ("basic", _swap((_Y3, "Offset(pgru1.y_t, -3)")),
                                     ["cycle at node pgru1.y2_t", "its recurrent input pgru1.y_t is not inside IfDefined()"]),
    "gates over different x": ("basic", _swap((_RPRE, _RPRE.replace("Append(tdnn2.batchnorm,", "Append(Scale(0.5, tdnn2.batchnorm),"))),
                               ["cycle at node pgru1.r_t_pre", "the two gates do not read the same feed-forward input"]),
    "y2_t reading the wrong gate": ("basic", _swap((_Y2, _Y2.replace("pgru1.z_t)", "pgru1.h_t)"))),
                                    ["cycle at node pgru1.y2_t", "its second input is not the update gate pgru1.z_t that y1_t reads"]),
    "y2_t reading the state of gru-layer": ("plain", _swap(("input=Append(" + _S3 + ", pgru1.z_t)", "input=Append(" + _Y3 + ", pgru1.z_t)")),
                                            ["cycle at node pgru1.y2_t", "the product y2_t reads pgru1.y_t, not pgru1.s_t as in gru-layer"]),
    "a weight of the wrong shape": ("basic", _swap((_RPRE, _RPRE.replace("component=pgru1.W_z.xs_r", "component=pgru1.W_z.xs_z"))),
                                    ["cycle at node pgru1.r_t_pre", "the gate's affine has 32 rows, not the recurrent dim 8"]),
    "an inner node read from outside": ("basic", _add_nodes(["dim-range-node name=pgru1.zz input-node=pgru1.z_t dim-offset=0 dim=16"],
                                                            (_TDNN3, _TDNN3.replace(", pgru1.sn_t,", ", Sum(pgru1.sn_t, pgru1.zz),"))),
                                        ["cycle at node pgru1.z_t", "the node is read from outside the block, by pgru1.zz"]),
    "a second NoOp node": ("basic", _add_nodes(["component-node name=pgru1.y_b component=pgru1.y input=pgru1.y_t"],
                                               ("component=pgru1.W_s.ys input=pgru1.y_t", "component=pgru1.W_s.ys input=pgru1.y_b")),
                           ["cycle at node pgru1.y_", "a second NoOpComponent node in one cycle"]),
    "normalize with add-log-stddev": ("onorm", _swap(("<AddLogStddev> F", "<AddLogStddev> T")),
                                      ["cycle at node gru1.s_t_preclip_renorm", "a NormalizeComponent with add-log-stddev=true is not supported"]),
    "the output product the other way round": ("onorm", _swap(("input=Append(gru1.o_t, gru1.y_t)", "input=Append(gru1.y_t, gru1.o_t)")),
                                               ["cycle at node gru1.y_o_t", "the product's input is not Append(o_t, y_t)"]),
    "the per-element scale over the state": ("onorm", _swap(("component=gru1.W_h.UW_elementwise input=IfDefined(Offset(gru1.y_t, -3))",
                                                             "component=gru1.W_h.UW_elementwise input=IfDefined(Offset(gru1.y_o_t, -3))")),
                                             ["cycle at node gru1.h_t_pre2", "the per-element scale h_t_pre2 reads gru1.y_o_t, not gru1.y_t"]),
}
_SRC = {"basic": None, "plain": _PLAIN_TEXT, "onorm": _ONORM_TEXT}


def _refused_model(built, tmp_path, what):
    which, edit, needles = REFUSED[what]
    src = built("gc_text")[:2] if which == "basic" else cases.build_case_files(_SRC[which], tmp_path / "src")[:2]
    return _edited(src, tmp_path, edit), needles


@pytest.mark.parametrize("what", list(REFUSED))
def test_cycles_that_are_no_composed_gru_block_are_refused(built, tmp_path, what):
    """A cycle that holds a NoOpComponent node and none of the nonlinearity components, and is not exactly what one of the five layers
    emits, is refused at load with the node and the reason, in a sentence of its own that names the five layers: gc_text's (or the
    gru-layer's, the norm-opgru-layer's) config text with one thing changed."""
    from rhasspy_speech_amd import _lib
    (dst, gd), needles = _refused_model(built, tmp_path, what)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    msg = str(ei.value)
    assert "a recurrent cycle without a nonlinearity component but with a NoOpComponent node is supported only as " + FIVE in msg, msg
    for needle in needles:
        assert needle in msg, (needle, msg)


def test_a_const_outside_such_a_block_is_refused(built, tmp_path):
    """Const() has no node behind it: anywhere but in the (1 - z_t) of a composed block it is refused by name, not read as a node."""
    from rhasspy_speech_amd import _lib
    dst, gd = _edited(built("gc_text")[:2], tmp_path, _swap((_TDNN3, _TDNN3.replace(", pgru1.sn_t,", ", Sum(pgru1.sn_t, Const(1, 16)),"))))
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(dst, gd)
    assert "Const() in the input of node tdnn3.affine is supported only as the Sum(Scale(-1.0, z_t), Const(1.0, cell-dim))" in str(ei.value), str(ei.value)


def _refused(case, root, needle):
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = cases.build_case_files(case, root)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert needle in str(ei.value), str(ei.value)


def test_sizes_beyond_the_kernels_limits_fail_the_load(tmp_path):
    """The limits are the fast blocks': cell <= 2048, R + P <= 4096, 144 KiB of LDS; gru-layer above cell dim 752 stays refused."""
    from rhasspy_speech_amd import _lib
    big = dict(spec=gc._net((gc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(big, tmp_path / "cell", "recurrent block pgru1.y_t: cell dim 2304 is more than the 2048 the HIP kernel takes")
    out = dict(spec=gc._net(gru=(gc._b(cell=32, rec=8, nonrec=4100, norm=True),)), graph="grammar", audio="zeros:0")
    _refused(out, tmp_path / "out", "recurrent block gru1.y_t: output dim 4108 (recurrent + non-recurrent) is more than the 4096 the HIP kernel takes")
    # 64 bytes x (three tiles of 512 + 4 and one of 2048 + 4 floats)
    lds = dict(spec=gc._net((gc._b(cell=2048, rec=512, nonrec=16),)), graph="grammar", audio="zeros:0")
    _refused(lds, tmp_path / "lds", "recurrent block pgru1.y_t: the state, product and cell rows of 16 chains (cell dim 2048, recurrent dim 512, 230400 bytes) "
                                    "do not fit the 147456 bytes of LDS the HIP kernel keeps them in")
    plain = dict(spec=gc._net((gc._plain(cell=768),)), graph="grammar", audio="zeros:0")
    _refused(plain, tmp_path / "plain", "recurrent block pgru1.y_t: the state, product and cell rows of 16 chains (cell dim 768, recurrent dim 768, 148224 bytes) "
                                        "do not fit the 147456 bytes of LDS the HIP kernel keeps them in")
    fits = dict(spec=gc._net((gc._plain(cell=752),)), graph="grammar", audio="zeros:0")
    md, gd, _, _ = cases.build_case_files(fits, tmp_path / "fits")
    assert " cell=752 rec=0 nonrec=0 " in _lib.Model(md, gd).describe()


def test_text_and_binary_models_are_the_same_network(built):
    from rhasspy_speech_amd import _lib
    a = _lib.Model(*built("gc_pgru")[:2]).describe()
    b = _lib.Model(*built("gc_text")[:2]).describe()
    keep = ("op:", "pgru:", "gru:", "nnet:")
    assert [l for l in a.splitlines() if l.startswith(keep)] == [l for l in b.splitlines() if l.startswith(keep)]


# ------------------------------------------------------------------------------------------ reader, recogniser and planners under sanitizers

def test_reader_and_planners_under_sanitizers(built, tmp_path):
    """tests/host/gruc_plan_check.cc (its own main; address + undefined-behaviour sanitizers, nothing loaded into Python) reads every
    case's final.mdl and every edited model of the refusal table, compiles the network and plans every GRU block; what it prints is
    what describe() says, or the refusal.  A recipe-size block of either family plans inside the kernels' 144 KiB of LDS."""
    from rhasspy_speech_amd import _lib, synth
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "gruc_plan_check"
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "gruc_plan_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc", CSRC / "nnet3_setup.cc", CSRC / "pgru_plan.cc", CSRC / "gru_plan.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(srcs)
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args, want = [], []
    for name in gc.CASES:
        args += [name, str(_mdl(built(name)[0]))]
        if name in gc.NO_GOLDEN:      # (the dither rule is the engine's, not the reader's: the network itself plans like gc_pgru's)
            want += [f"{name} {l}" for l in _block_lines(name, "pgru")]
        else:
            text = _lib.Model(*built(name)[:2]).describe()      # (describe groups the lines by kind; the program prints in network order)
            line_of = {l.split()[1]: l for l in text.splitlines() if l.startswith(("lstm: ", "gru: ", "pgru: "))}
            for op in [l for l in text.splitlines() if l.startswith(("op: lstm ", "op: gru ", "op: pgru "))]:
                l = line_of[op.split()[2]]
                want.append(f"{name} {l.split()[0]} {l.split()[1]}" if l.startswith("lstm: ") else f"{name} {l}")
    for i, what in enumerate(REFUSED):
        (dst, _gd), needles = _refused_model(built, tmp_path / f"refused{i}", what)
        args += [f"r{i}", str(_mdl(dst))]
        want.append((f"r{i} error: ", needles))
    full_p = "input=32 cell=1024 rec=256 nonrec=256 delay=3 scale=1 norm={n} dropout=0 kernel=pgruc16x16x4<w8> rows_per_block=16 lds=115712 w_zr=32+256 " \
             "cell_tiles=64 rec_tiles=16 out_tiles=32 grid=chains/16 form=composed"
    full_g = "input=32 cell=1024 rec=256 nonrec=256 delay=3 scale=1 norm={n} dropout=0 kernel=gruc16x16x4<w8> rows_per_block=16 lds=99072 w_zo=32+256 " \
             "cell_tiles=64 out_tiles=32 grid=chains/16 form=composed"
    assert 64 * (3 * 260 + 1028) == 115712 <= 144 * 1024 and 64 * (2 * 260 + 1028) == 99072
    extra = {
        "x_full_pgru": (dict(spec=gc._net((gc._b(cell=1024, rec=256, nonrec=256),)), graph="grammar", audio="zeros:0"), "x_full_pgru pgru: pgru1.y_t " + full_p.format(n=0)),
        "x_full_npgru": (dict(spec=gc._net((gc._b(cell=1024, rec=256, nonrec=256, norm=True),)), graph="grammar", audio="zeros:0"),
                         "x_full_npgru pgru: pgru1.y_t " + full_p.format(n=1)),
        "x_full_opgru": (dict(spec=gc._net(gru=(gc._b(cell=1024, rec=256, nonrec=256),)), graph="grammar", audio="zeros:0"), "x_full_opgru gru: gru1.y_t " + full_g.format(n=0)),
        "x_cell": (dict(spec=gc._net(gru=(gc._b(cell=2304, rec=16, nonrec=16),)), graph="grammar", audio="zeros:0"),
                   "x_cell error: nnet3: recurrent block gru1.y_t: cell dim 2304 is more than the 2048 the HIP kernel takes"),
    }
    for name, (case, line) in extra.items():
        mdl = tmp_path / name / "final.mdl"
        synth.write_final_mdl(mdl, cases.case_spec(case))
        args += [name, str(mdl)]
        want.append(line)
    p = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    got = p.stdout.splitlines()
    assert len(got) == len(want), p.stdout
    for g, w in zip(got, want):
        if isinstance(w, tuple):
            assert g.startswith(w[0]) and FIVE in g and all(n in g for n in w[1]), (g, w)
        else:
            assert g == w, (g, w)


# ------------------------------------------------------------------------------------------ the synthetic model writer

def test_block_nodes_are_written_in_xconfig_s_order():
    """The config lines of a composed block in the order XconfigGruLayer / XconfigPgruLayer / XconfigNormPgruLayer / XconfigOpgruLayer
    / XconfigNormOpgruLayer emit them (xconfig/gru.py), and the components' names and order."""
    from rhasspy_speech_amd import synth

    def names(case, what):
        spec = cases.case_spec(gc.CASES[case])
        return [l.split("name=")[1].split()[0].split(".", 1)[1] for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if f" name={what}." in l]

    def comps(case, what):
        spec = cases.case_spec(gc.CASES[case])
        return [n.split(".", 1)[1] for n, _ in synth.build_nnet(spec, np.random.default_rng(spec.seed))[1] if n.startswith(what + ".")]
    cell = ["z_t_pre", "z_t", "r_t_pre", "r_t", "h1_t", "h_t_pre", "h_t", "y1_t", "y2_t", "y_t"]
    assert names("gc_gru", "pgru1") == cell + ["s_t"]
    assert names("gc_pgru", "pgru1") == cell + ["sn_t", "s_t_preclip", "s_t"]
    assert names("gc_npgru_drop", "pgru1") == ["z_t_pre", "z_predrop_t", "z_t", "r_t_pre", "r_predrop_t", "r_t"] + cell[4:] + \
        ["sn_nobatchnorm_t", "s_t_preclip", "sn_t", "s_renorm_t", "s_t"]
    ocell = ["z_t_pre", "z_t", "o_t_pre", "o_t", "h_t_pre", "h_t_pre2", "h_t", "y1_t", "y2_t", "y_t", "y_o_t"]
    assert names("gc_opgru", "gru1") == ocell + ["sn_t", "s_t_preclip", "s_t"]
    assert names("gc_nopgru_drop", "gru1") == ["z_t_pre", "z_predrop_t", "z_t", "o_t_pre", "o_predrop_t", "o_t"] + ocell[4:] + \
        ["sn_nobatchnorm_t", "sn_t", "s_t_preclip", "s_t_preclip_renorm", "s_t"]
    assert comps("gc_gru", "pgru1") == ["W_z.xs_z", "W_z.xs_r", "W_h.UW", "z", "r", "h", "h1", "y1", "y2", "y", "s_r"]
    assert comps("gc_pgru", "pgru1") == ["W_z.xs_z", "W_z.xs_r", "W_h.UW", "z", "r", "h", "h1", "y1", "y2", "y", "W_s.ys", "s_r"]
    assert comps("gc_npgru_drop", "pgru1") == ["W_z.xs_z", "W_z.xs_r", "W_h.UW", "dropout_z", "dropout_r", "z", "r", "h", "h1", "y1", "y2", "y", "W_s.ys", "s_r",
                                               "batchnorm", "renorm"]
    assert comps("gc_opgru", "gru1") == ["W_z.xs_z", "W_z.xs_o", "W_h.UW", "W_h.UW_elementwise", "z", "o", "h", "o1", "y1", "y2", "y", "W_s.ys", "s_r"]
    assert comps("gc_nopgru_drop", "gru1") == ["W_z.xs_z", "W_z.xs_o", "W_h.UW", "W_h.UW_elementwise", "z", "o", "h", "o1", "y1", "y2", "y", "dropout", "W_s.ys", "s_r",
                                                "batchnorm", "renorm"]
    spec = cases.case_spec(gc.CASES["gc_pgru"])
    y1 = [l for l in synth.build_nnet(spec, np.random.default_rng(spec.seed))[0] if " name=pgru1.y1_t " in l]
    assert y1 == ["component-node name=pgru1.y1_t component=pgru1.y1 input=Append(pgru1.h_t, Sum(Scale(-1, pgru1.z_t), Const(1, 32)))"]
    for bad in (dict(after=2, cell=32, rec=8, nonrec=8, form="slow"),):
        with pytest.raises(ValueError):
            synth._gru_form(bad)
    assert synth.tiny_spec().gru_layers == () and synth.tiny_spec().pgru_layers == ()


# what the parent's synth.py wrote for these cases of tests/pgru_cases.py and tests/gru_cases.py (sha256 of final.mdl)
_FAST_FILES = {
    (pc, "pg_basic"): "3da2098de17f2b84d0930a0a723bb95c9b1ff901296263119faee3433e967655",
    (pc, "pg_plain"): "c8fd2661a84536b1ad03d82671a98d2262f09a3368c73bbb633109a093466397",
    (pc, "pg_norm_drop"): "d59fae5fd2b5edf9c9c25d696e3d1eddbc342a9cd72dfb5f861c13d417704884",
    (pc, "pg_text"): "3945d8590d1f88264646c7bf48df3ff5d99a290ea5171d8813b837e97c244951",
    (pc, "pg_mixed"): "7c7640e9abd695d27abf8ee3b205333a60744f6f38d7137442783dad62460f28",
    (grc, "gr_basic"): "8cb909e0ca4c9bdd72de37a3c5bcde3cbc607936765c24ee3762d467b4c62b46",
    (grc, "gr_norm_drop"): "2b7c44fb20300d815fb956b173513edb654ea22cb1583c48424cb69564eb6814",
}


def test_fast_form_model_files_are_byte_identical(tmp_path):
    """With `form` absent -- and with form="fast" spelled out -- the files written for the fast cases are byte for byte what they were
    before the composed writers existed."""
    import dataclasses
    from rhasspy_speech_amd import synth
    for (mod, name), digest in _FAST_FILES.items():
        spec = cases.case_spec(mod.CASES[name])
        synth.write_final_mdl(tmp_path / f"{name}.mdl", spec)
        assert hashlib.sha256((tmp_path / f"{name}.mdl").read_bytes()).hexdigest() == digest, name
        fast = dataclasses.replace(spec, gru_layers=tuple(dict(l, form="fast") for l in spec.gru_layers),
                                   pgru_layers=tuple(dict(l, form="fast") for l in spec.pgru_layers))
        synth.write_final_mdl(tmp_path / f"{name}_fast.mdl", fast)
        assert (tmp_path / f"{name}_fast.mdl").read_bytes() == (tmp_path / f"{name}.mdl").read_bytes(), name
