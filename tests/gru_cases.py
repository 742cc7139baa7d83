"""TDNN-OPGRU models (nnet3's fast-opgru-layer / fast-norm-opgru-layer: OutputGruNonlinearityComponent between Sigmoid,
ElementwiseProduct, Normalize and BackpropTruncation components): the case table of tests/test_gru_cpu.py, tests/test_gpu_gru.py and
tests/gen_gru_golden.py, and a float64 numpy restatement of the case networks on top of lstm_cases.Float64Net.  Tiny specs as in
tests/lstm_cases.py (24 phones, 48 pdfs, hidden width 32; clips of 1-2 s); what the reference's two decoder binaries and rs-dump gave
for each is in tests/golden/gru/<case>.npz."""
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests import lstm_cases as lc

GOLDEN = cases.GOLDEN / "gru"
NBEST = cases.NBEST

_TDNN = ((0,), (-1, 0, 1), (-3, 0, 3))


def _gr(layers, dither=0.0, layer_offsets=_TDNN, **spec):
    s = dict(ivector_dim=0, dither=dither, layer_offsets=layer_offsets, gru_layers=tuple(layers))
    s.update(spec)
    return s


def _b(after=2, cell=32, rec=8, nonrec=8, delay=3, **kw):
    return dict(after=after, cell=cell, rec=rec, nonrec=nonrec, delay=delay, **kw)


_BASIC = (_b(),)

CASES = {
    # tdnn(0), tdnn(-1,0,1), OPGRU C=32 R=8 P=8 delay 3, tdnn(-3,0,3), output
    "gr_basic": dict(spec=_gr(_BASIC), graph="grammar", audio="synth:70:24000"),
    # nothing a multiple of 16, R != P, delay 1
    "gr_odd": dict(spec=_gr((_b(cell=20, rec=6, nonrec=10, delay=1),)), graph="grammar", audio="synth:71:24000"),
    # fast-norm-opgru-layer: NormalizeComponent in the recurrence, BatchNorm on the output
    "gr_norm": dict(spec=_gr((_b(norm=True),)), graph="grammar", audio="synth:72:24000"),
    # ... with dropout-proportion given: one DropoutComponent behind both sigmoids (a copy in test mode)
    "gr_norm_drop": dict(spec=_gr((_b(norm=True, dropout=True),)), graph="grammar", audio="synth:73:24000"),
    # decay-time=40 at delay 3: the truncation component scales the state by 0.925
    "gr_decay": dict(spec=_gr((_b(scale=0.925),)), graph="grammar", audio="synth:74:24000"),
    # ten cell tiles on eight waves, several k-steps in both products, several output tiles
    "gr_wide": dict(spec=_gr((_b(cell=160, rec=48, nonrec=48),)), graph="grammar", audio="synth:76:16000"),
    # the largest delay
    "gr_d8": dict(spec=_gr((_b(delay=8),)), graph="grammar", audio="synth:78:24000"),
    # GRU, tdnn(-3,0,3), norm-GRU with another shape and a scale, tdnn(-3,0,3); the iVector extractor is on
    "gr_stack": dict(spec=_gr((_b(), _b(after=3, cell=24, rec=8, nonrec=16, norm=True, scale=0.925)), layer_offsets=_TDNN + ((-3, 0, 3),), ivector_dim=10),
                     graph="grammar", audio="synth:89:32000"),
    # an LSTM block behind the second TDNN layer and a GRU block behind the third: result matrix 64 + k counts both
    "gr_mixed": dict(spec=_gr((_b(after=3),), lstm_layers=(dict(after=2, cell=32, rec=8, nonrec=8, delay=3),)), graph="grammar", audio="synth:84:24000"),
    # --frame-subsampling-factor=3: delay 3 under offsets {-3, 0, 3} is one residue class, delay 2 all three
    "gr_fsf3": dict(spec=_gr(_BASIC), graph="grammar", audio="synth:77:32000", conf_opts={"frame-subsampling-factor": 3}),
    "gr_fsf3_d2": dict(spec=_gr((_b(delay=2),)), graph="grammar", audio="synth:88:32000", conf_opts={"frame-subsampling-factor": 3}),
    "gr_text": dict(spec=_gr(_BASIC, binary=False), graph="grammar", audio="synth:70:24000"),
    # lengths on gr_basic's model: no frame, one frame, two frames (fewer than the delay), one frame more than a chunk of 24, one
    # fewer than two chunks
    "gr_len0": dict(spec=_gr(_BASIC), graph="grammar", audio="synth:79:399"),
    "gr_len1": dict(spec=_gr(_BASIC), graph="grammar", audio="synth:79:400"),
    "gr_len2": dict(spec=_gr(_BASIC), graph="grammar", audio="synth:79:560"),
    "gr_len25": dict(spec=_gr(_BASIC), graph="grammar", audio=f"synth:80:{400 + 24 * 160}"),
    "gr_len47": dict(spec=_gr(_BASIC), graph="grammar", audio=f"synth:81:{400 + 46 * 160}"),
    # no --dither line: the reference's set-up accepts the model, this library refuses it (the rand() position of a recurrent
    # compilation is not replayed)
    "gr_dither_default": dict(spec=_gr(_BASIC, dither=None), graph="grammar", audio="synth:70:24000"),
}
NO_GOLDEN = ("gr_dither_default",)
LENGTHS = ("gr_len0", "gr_len1", "gr_len2", "gr_len25", "gr_len47")


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


def block_dims(name: str):
    """Per recurrent block of the case, in network order: ("lstm", k, input dim, output dim, layer) or ("gru", k, input dim, output
    dim, layer), k counting the blocks of that kind from 1 as synth.py names them."""
    spec = cases.case_spec(CASES[name])
    out = []
    for after in range(1, len(spec.layer_offsets) + 1):
        in_dim = spec.hidden_dim
        for kind, layers, dims in (("lstm", spec.lstm_layers, synth.lstm_layer_dims), ("gru", spec.gru_layers, synth.gru_layer_dims)):
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

K_SQUARED_NORM_FLOOR = 2.0 ** -66      # NormalizeComponent::kSquaredNormFloor


class Float64Net(lc.Float64Net):
    """lstm_cases.Float64Net with the GRU block: OutputGruNonlinearityComponent::Propagate (nnet-combined-component.cc:1946-1985)
    between VectorBase::Sigmoid / Tanh, MulElements, the affine W_y, NormalizePerRow (cu-math.cc:302-310) in the norm variant and the
    truncation component's scale.  A chain starts where the block's feed-forward input first exists, with zeros before."""

    def _node(self, name):
        if name not in self.memo and re.match(r"^gru\d+\.", name):
            b = name.split(".", 1)[0]
            if not (name == f"{b}.y_t" and f"{b}.y_t_tmp" in self.nodes):      # (the norm variant's BatchNorm is an ordinary layer)
                self._gru_block(b)
                return self.memo[name]
        return super()._node(name)

    def _gru_block(self, b):
        nodes, comps = self.nodes, self.comps
        m = re.match(r"^Append\((.*), IfDefined\(Offset\((\S+), (-?\d+)\)\)\)$", nodes[f"{b}.z_t_pre"]["input"])
        x_desc, d = m.group(1), -int(m.group(3))
        assert m.group(2) == f"{b}.s_t" and nodes[f"{b}.hpart_t"]["input"] == x_desc
        t0, x = self._desc(x_desc)

        def aff(node):
            f = comps[nodes[node]["component"]][1]
            return f["<LinearParams>"][0].astype(np.float64), f["<BiasParams>"][0].astype(np.float64)

        (Wz, bz), (Wo, bo), (Wh, bh) = aff(f"{b}.z_t_pre"), aff(f"{b}.o_t_pre"), aff(f"{b}.hpart_t")
        norm = f"{b}.y_t_tmp" in nodes
        y_name = f"{b}.y_t_tmp" if norm else f"{b}.y_t"
        Wy, by = aff(y_name)
        w_h = comps[nodes[f"{b}.gru_nonlin_t"]["component"]][1]["<w_h>"][0].astype(np.float64)
        scale = float(np.float32(comps[nodes[f"{b}.s_t"]["component"]][1]["<Scale>"][0]))
        rms = float(np.float32(comps[nodes[f"{b}.s_t_renorm"]["component"]][1]["<TargetRms>"][0])) if norm else 1.0
        in_dim, C = x.shape[1], w_h.shape[0]
        R = Wz.shape[1] - in_dim
        n = x.shape[0]
        h = np.zeros((n, C)); c = np.zeros((n, C)); y = np.zeros((n, Wy.shape[0])); s = np.zeros((n, R))
        pre_z, pre_o, hp = x @ Wz[:, :in_dim].T + bz, x @ Wo[:, :in_dim].T + bo, x @ Wh.T + bh
        for i in range(n):
            sp = s[i - d] if i >= d else np.zeros(R)
            cp = c[i - d] if i >= d else np.zeros(C)
            z = lc._sigmoid(pre_z[i] + Wz[:, in_dim:] @ sp)
            o = lc._sigmoid(pre_o[i] + Wo[:, in_dim:] @ sp)
            h[i] = lc._tanh(hp[i] + w_h * cp)
            c[i] = h[i] - z * h[i] + z * cp
            y[i] = Wy @ (c[i] * o) + by
            r = y[i][:R]
            if norm:
                r = r * max(K_SQUARED_NORM_FLOOR, float(r @ r) / (R * rms * rms)) ** -0.5
            s[i] = scale * r
        memo = self.memo
        memo[f"{b}.gru_nonlin_t"] = (t0, np.concatenate([h, c], axis=1))
        memo[f"{b}.c_t"] = (t0, c)
        memo[y_name] = (t0, y)
        memo[f"{b}.s_t"] = (t0, s)

    def forward(self, feats, ivector=None):
        """As lstm_cases.Float64Net.forward; the second result holds the output rows of every recurrent block of either kind in
        network order -- an LSTM block's rp (or m), a GRU block's y before any BatchNorm."""
        ll, _ = super().forward(feats, ivector)
        T, blocks = feats.shape[0], []
        for name in self.nodes:
            b = name.rsplit(".", 1)[0]
            if name.endswith(".lstm_nonlin"):
                key = f"{b}.rp" if f"{b}.rp" in self.nodes else f"{b}.m"
            elif name.endswith(".gru_nonlin_t"):
                key = f"{b}.y_t_tmp" if f"{b}.y_t_tmp" in self.nodes else f"{b}.y_t"
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
