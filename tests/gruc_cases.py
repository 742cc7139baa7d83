"""TDNN-GRU models whose cell is spelled out as separate components (nnet3's gru-layer / pgru-layer / norm-pgru-layer / opgru-layer /
norm-opgru-layer: Sigmoid, Tanh, ElementwiseProduct and NoOp nodes, no GruNonlinearityComponent): the case table of
tests/test_gruc_cpu.py, tests/test_gpu_gruc.py and tests/gen_gruc_golden.py, and a float64 numpy restatement of the composed blocks
on top of gru_cases.Float64Net (through pgru_cases.Float64Net: one case mixes a fast block in).  Tiny specs as in tests/gru_cases.py
(24 phones, 48 pdfs, hidden width 32; clips of 1-2 s); what the reference's two decoder binaries and rs-dump gave for each is in
tests/golden/gruc/<case>.npz."""
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests import gru_cases as gc
from tests import lstm_cases as lc
from tests import pgru_cases as pc

GOLDEN = cases.GOLDEN / "gruc"
NBEST = cases.NBEST

_TDNN = ((0,), (-1, 0, 1), (-3, 0, 3))


def _net(pgru=(), gru=(), dither=0.0, layer_offsets=_TDNN, **spec):
    s = dict(ivector_dim=0, dither=dither, layer_offsets=layer_offsets, pgru_layers=tuple(pgru), gru_layers=tuple(gru))
    s.update(spec)
    return s


def _b(after=2, cell=32, rec=8, nonrec=8, delay=3, form="composed", **kw):
    return dict(after=after, cell=cell, rec=rec, nonrec=nonrec, delay=delay, form=form, **kw)


def _plain(after=2, cell=32, delay=3, **kw):
    return dict(after=after, cell=cell, rec=0, nonrec=0, delay=delay, form="composed", **kw)


_BASIC = (_b(),)

CASES = {
    # ---- the reset-gate family.  tdnn(0), tdnn(-1,0,1), pgru-layer C=32 R=8 P=8 delay 3, tdnn(-3,0,3), output
    "gc_pgru": dict(spec=_net(_BASIC), graph="grammar", audio="synth:200:24000"),
    # gru-layer: no projection, s_t = s_r(y_t) is output and recurrence, y2_t reads the scaled state
    "gc_gru": dict(spec=_net((_plain(),)), graph="grammar", audio="synth:201:24000"),
    # norm-pgru-layer: NormalizeComponent in the recurrence, BatchNorm on the output
    "gc_npgru": dict(spec=_net((_b(norm=True),)), graph="grammar", audio="synth:202:24000"),
    # ... with dropout-proportion given: a DropoutComponent behind each sigmoid (copies in test mode)
    "gc_npgru_drop": dict(spec=_net((_b(norm=True, dropout=True),)), graph="grammar", audio="synth:203:24000"),
    # nothing a multiple of 16, R != P, delay 1
    "gc_pgru_odd": dict(spec=_net((_b(cell=20, rec=6, nonrec=10, delay=1),)), graph="grammar", audio="synth:204:24000"),
    # ten cell tiles on eight waves, three r tiles, several k-steps in all three products, several output tiles
    "gc_pgru_wide": dict(spec=_net((_b(cell=160, rec=48, nonrec=48),)), graph="grammar", audio="synth:205:16000"),
    # gru-layer with nine cell tiles on eight waves: the state rows are 144 wide
    "gc_gru_wide": dict(spec=_net((_plain(cell=144),)), graph="grammar", audio="synth:206:16000"),
    # decay-time=40 at delay 3: the truncation component scales the state by 0.925; y_t is read back unscaled
    "gc_pgru_decay": dict(spec=_net((_b(scale=0.925),)), graph="grammar", audio="synth:207:24000"),
    # ---- the output-gate family.  opgru-layer, norm-opgru-layer, the latter with its one shared DropoutComponent
    "gc_opgru": dict(spec=_net(gru=_BASIC), graph="grammar", audio="synth:208:24000"),
    "gc_nopgru": dict(spec=_net(gru=(_b(norm=True),)), graph="grammar", audio="synth:209:24000"),
    "gc_nopgru_drop": dict(spec=_net(gru=(_b(norm=True, dropout=True),)), graph="grammar", audio="synth:210:24000"),
    "gc_opgru_odd": dict(spec=_net(gru=(_b(cell=20, rec=6, nonrec=10, delay=1),)), graph="grammar", audio="synth:211:24000"),
    "gc_opgru_wide": dict(spec=_net(gru=(_b(cell=160, rec=48, nonrec=48),)), graph="grammar", audio="synth:212:16000"),
    # the largest delay
    "gc_opgru_d8": dict(spec=_net(gru=(_b(delay=8),)), graph="grammar", audio="synth:213:24000"),
    # pgru-layer, tdnn(-3,0,3), norm-opgru-layer with another shape and a scale, tdnn(-3,0,3); the iVector extractor is on
    "gc_stack": dict(spec=_net(_BASIC, gru=(_b(after=3, cell=24, rec=8, nonrec=12, norm=True, scale=0.925),), layer_offsets=_TDNN + ((-3, 0, 3),),
                               ivector_dim=10), graph="grammar", audio="synth:214:32000"),
    # an LSTM and a composed opgru block behind the second TDNN layer and a fast-pgru block behind the third: result matrix 64 + k
    # counts all of them in network order
    "gc_mixed": dict(spec=_net((_b(after=3, form="fast"),), gru=_BASIC, lstm_layers=(dict(after=2, cell=32, rec=8, nonrec=8, delay=3),)),
                     graph="grammar", audio="synth:215:24000"),
    # --frame-subsampling-factor=3: delay 3 under offsets {-3, 0, 3} is one residue class, delay 2 all three
    "gc_fsf3": dict(spec=_net(_BASIC), graph="grammar", audio="synth:216:32000", conf_opts={"frame-subsampling-factor": 3}),
    "gc_fsf3_d2": dict(spec=_net(gru=(_b(delay=2),)), graph="grammar", audio="synth:217:32000", conf_opts={"frame-subsampling-factor": 3}),
    "gc_text": dict(spec=_net(_BASIC, binary=False), graph="grammar", audio="synth:200:24000"),
    # lengths on gc_pgru's model: no frame, one frame, two frames (fewer than the delay), one frame more than a chunk of 24, one
    # fewer than two chunks
    "gc_len0": dict(spec=_net(_BASIC), graph="grammar", audio="synth:218:399"),
    "gc_len1": dict(spec=_net(_BASIC), graph="grammar", audio="synth:218:400"),
    "gc_len2": dict(spec=_net(_BASIC), graph="grammar", audio="synth:218:560"),
    "gc_len25": dict(spec=_net(_BASIC), graph="grammar", audio=f"synth:219:{400 + 24 * 160}"),
    "gc_len47": dict(spec=_net(_BASIC), graph="grammar", audio=f"synth:220:{400 + 46 * 160}"),
    # no --dither line: the reference's set-up accepts the model, this library refuses it (the rand() position of a recurrent
    # compilation is not replayed)
    "gc_dither_default": dict(spec=_net(_BASIC, dither=None), graph="grammar", audio="synth:200:24000"),
}
NO_GOLDEN = ("gc_dither_default",)
LENGTHS = ("gc_len0", "gc_len1", "gc_len2", "gc_len25", "gc_len47")


def model_key(name: str):
    """Cases with the same key decode with one model and one graph."""
    c = CASES[name]
    return repr((sorted(c["spec"].items(), key=str), c["graph"], c.get("conf_opts"), c.get("opts")))


def build_case_files(name: str, root: Path):
    """(model_dir, graph_dir, wav, pcm) of the case under `root`."""
    return cases.build_case_files(CASES[name], root)


def load_golden(name: str):
    return np.load(GOLDEN / f"{name}.npz")


def fsf_of(name: str) -> int:
    return int(CASES[name].get("conf_opts", {}).get("frame-subsampling-factor", 1))


def is_composed(layer) -> bool:
    return layer.get("form", "fast") == "composed"


def block_dims(name: str):
    """Per recurrent block of the case, in network order: (kind, k, input dim, output dim, layer) with kind one of "lstm", "gru",
    "pgru" and k counting the blocks of that kind from 1 as synth.py names them."""
    spec = cases.case_spec(CASES[name])
    out = []
    for after in range(1, len(spec.layer_offsets) + 1):
        in_dim = spec.hidden_dim
        for kind, layers, dims in (("lstm", spec.lstm_layers, synth.lstm_layer_dims), ("gru", spec.gru_layers, synth.gru_layer_dims),
                                   ("pgru", spec.pgru_layers, synth.pgru_layer_dims)):
            for k, layer in enumerate(layers, start=1):
                if int(layer["after"]) == after:
                    out.append((kind, k, in_dim, dims(layer)[3], layer))
                    in_dim = dims(layer)[3]
    return out


def contexts(name: str):
    """(left, right) context of the case's network: the offsets' sums through the feed-forward layers (ComputeSimpleNnetContext
    ignores the optional recurrent dependency)."""
    spec = cases.case_spec(CASES[name])
    return (-min(spec.lda_offsets) + sum(-min(o) for o in spec.layer_offsets), max(spec.lda_offsets) + sum(max(o) for o in spec.layer_offsets))


# ------------------------------------------------------------------------------------------ float64 restatement

class Float64Net(pc.Float64Net):
    """gru_cases.Float64Net (with pgru_cases' fast block) and the composed GRU cells, node by node as xconfig/gru.py wires them:
    VectorBase::Sigmoid / Tanh, the ElementwiseProductComponents h1, y1, y2 and o1, Sum(Scale(-1, z_t), Const(1)), the per-element
    scale W_h.UW_elementwise, the affine W_s.ys, NormalizePerRow (cu-math.cc:302-310) in the norm forms and the truncation component's
    scale; in gru-layer the state is the scaled cell and y2_t reads it.  A chain starts where the block's feed-forward input first
    exists, with zeros before."""

    def _composed(self, b):
        return f"{b}.y1_t" in self.nodes

    def _node(self, name):
        if name not in self.memo and re.match(r"^p?gru\d+\.", name):
            b = name.split(".", 1)[0]
            if self._composed(b):
                if name == f"{b}.sn_t" and f"{b}.sn_nobatchnorm_t" in self.nodes:      # (the norm forms' BatchNorm is an ordinary layer)
                    return lc.Float64Net._node(self, name)
                self._composed_block(b)
                return self.memo[name]
        return super()._node(name)

    def _composed_block(self, b):
        nodes, comps = self.nodes, self.comps
        m = re.match(r"^Append\((.*), IfDefined\(Offset\((\S+), (-?\d+)\)\)\)$", nodes[f"{b}.z_t_pre"]["input"])
        x_desc, d = m.group(1), -int(m.group(3))
        assert m.group(2) == f"{b}.s_t"
        one_minus = re.match(r"^Append\((\S+), Sum\(Scale\((\S+), (\S+)\), Const\((\S+), (\d+)\)\)\)$", nodes[f"{b}.y1_t"]["input"])
        assert one_minus and one_minus.group(1) == f"{b}.h_t" and one_minus.group(3) == f"{b}.z_t"
        z_scale, const = float(one_minus.group(2)), float(one_minus.group(4))
        t0, x = self._desc(x_desc)

        def aff(node):
            f = comps[nodes[node]["component"]][1]
            return f["<LinearParams>"][0].astype(np.float64), f["<BiasParams>"][0].astype(np.float64)

        out_gate = f"{b}.o_t_pre" in nodes
        (Wz, bz), (Wg, bg), (Wh, bh) = aff(f"{b}.z_t_pre"), aff(f"{b}.o_t_pre" if out_gate else f"{b}.r_t_pre"), aff(f"{b}.h_t_pre")
        norm = f"{b}.sn_nobatchnorm_t" in nodes
        proj = norm or f"{b}.sn_t" in nodes
        y_name = f"{b}.sn_nobatchnorm_t" if norm else f"{b}.sn_t"
        scale = float(np.float32(comps[nodes[f"{b}.s_t"]["component"]][1]["<Scale>"][0]))
        renorm = nodes[f"{b}.s_t"]["input"]
        rms = float(np.float32(comps[nodes[renorm]["component"]][1]["<TargetRms>"][0])) if norm else 1.0
        in_dim, C = x.shape[1], Wz.shape[0]
        R = Wz.shape[1] - in_dim
        y_prev_scaled = nodes[f"{b}.y2_t"]["input"].startswith(f"Append(IfDefined(Offset({b}.s_t,")      # gru-layer
        assert proj or (R == C and y_prev_scaled)
        if out_gate:
            w_h = comps[nodes[f"{b}.h_t_pre2"]["component"]][1]["<Params>"][0].astype(np.float64)
            assert Wh.shape == (C, in_dim) and Wg.shape == (C, in_dim + R)
        else:
            assert Wh.shape == (C, in_dim + R) and Wg.shape == (R, in_dim + R)
        if proj:
            Wy, by = aff(y_name)
        n = x.shape[0]
        h = np.zeros((n, C)); y = np.zeros((n, C)); s = np.zeros((n, R))
        sn = np.zeros((n, Wy.shape[0])) if proj else None
        pre_z, pre_g, pre_h = x @ Wz[:, :in_dim].T + bz, x @ Wg[:, :in_dim].T + bg, x @ Wh[:, :in_dim].T + bh
        for i in range(n):
            sp = s[i - d] if i >= d else np.zeros(R)
            yp = sp if y_prev_scaled else (y[i - d] if i >= d else np.zeros(C))
            z = lc._sigmoid(pre_z[i] + Wz[:, in_dim:] @ sp)
            g = lc._sigmoid(pre_g[i] + Wg[:, in_dim:] @ sp)
            if out_gate:
                h[i] = lc._tanh(pre_h[i] + w_h * yp)
            else:
                h[i] = lc._tanh(pre_h[i] + Wh[:, in_dim:] @ (g * sp))
            y[i] = h[i] * (z_scale * z + const) + yp * z
            if proj:
                sn[i] = Wy @ (g * y[i] if out_gate else y[i]) + by
                v = sn[i][:R]
                if norm:
                    v = v * max(gc.K_SQUARED_NORM_FLOOR, float(v @ v) / (R * rms * rms)) ** -0.5
                s[i] = scale * v
            else:
                s[i] = scale * y[i]
        memo = self.memo
        memo[f"{b}.y_t"] = (t0, y)
        memo[f"{b}.h_t"] = (t0, h)
        memo[f"{b}.s_t"] = (t0, s)
        if proj:
            memo[y_name] = (t0, sn)

    def forward(self, feats, ivector=None):
        """As gru_cases.Float64Net.forward; the second result holds the output rows of every recurrent block of any kind in network
        order -- a composed block's W_s.ys rows before any BatchNorm, the cell y_t of a gru-layer block."""
        ll, _ = lc.Float64Net.forward(self, feats, ivector)
        T, blocks = feats.shape[0], []
        for name in self.nodes:
            b = name.rsplit(".", 1)[0]
            if name.endswith(".lstm_nonlin"):
                key = f"{b}.rp" if f"{b}.rp" in self.nodes else f"{b}.m"
            elif name.endswith(".gru_nonlin_t"):
                key = f"{b}.y_t_tmp" if f"{b}.y_t_tmp" in self.nodes else f"{b}.y_t"
            elif name.endswith(".y1_t"):
                key = next(k for k in (f"{b}.sn_nobatchnorm_t", f"{b}.sn_t", f"{b}.y_t") if k in self.nodes)
            else:
                continue
            bt0, rows = self.memo[key]
            blocks.append(rows[-bt0:-bt0 + T])
        return ll, blocks


def restate(name: str, g=None):
    """(log-likelihoods as the reference lays them out, [block outputs, every frame]) of the case from its golden's input rows, in
    float64."""
    g = load_golden(name) if g is None else g
    spec = cases.case_spec(CASES[name])
    net = Float64Net(spec, *contexts(name))
    iv = g["offline_ivector"][0] if "offline_ivector" in g.files else None
    ll, blocks = net.forward(g["input"], iv)
    return ll[::fsf_of(name)], blocks
