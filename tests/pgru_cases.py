"""TDNN-PGRU / TDNN-GRU models (nnet3's fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer: GruNonlinearityComponent between
Sigmoid, Normalize and BackpropTruncation components): the case table of tests/test_pgru_cpu.py, tests/test_gpu_pgru.py and
tests/gen_pgru_golden.py, and a float64 numpy restatement of the case networks on top of gru_cases.Float64Net.  Tiny specs as in
tests/gru_cases.py (24 phones, 48 pdfs, hidden width 32; clips of 1-2 s); what the reference's two decoder binaries and rs-dump gave
for each is in tests/golden/pgru/<case>.npz."""
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests import gru_cases as gc
from tests import lstm_cases as lc

GOLDEN = cases.GOLDEN / "pgru"
NBEST = cases.NBEST

_TDNN = ((0,), (-1, 0, 1), (-3, 0, 3))


def _pg(layers, dither=0.0, layer_offsets=_TDNN, **spec):
    s = dict(ivector_dim=0, dither=dither, layer_offsets=layer_offsets, pgru_layers=tuple(layers))
    s.update(spec)
    return s


def _b(after=2, cell=32, rec=8, nonrec=8, delay=3, **kw):
    return dict(after=after, cell=cell, rec=rec, nonrec=nonrec, delay=delay, **kw)


def _plain(after=2, cell=32, delay=3, **kw):
    return dict(after=after, cell=cell, rec=0, nonrec=0, delay=delay, **kw)


_BASIC = (_b(),)

CASES = {
    # tdnn(0), tdnn(-1,0,1), PGRU C=32 R=8 P=8 delay 3, tdnn(-3,0,3), output
    "pg_basic": dict(spec=_pg(_BASIC), graph="grammar", audio="synth:170:24000"),
    # nothing a multiple of 16, R != P, delay 1
    "pg_odd": dict(spec=_pg((_b(cell=20, rec=6, nonrec=10, delay=1),)), graph="grammar", audio="synth:171:24000"),
    # fast-gru-layer: no projection, the state is the scaled cell
    "pg_plain": dict(spec=_pg((_plain(),)), graph="grammar", audio="synth:172:24000"),
    "pg_plain_odd": dict(spec=_pg((_plain(cell=20, delay=1),)), graph="grammar", audio="synth:173:24000"),
    # fast-norm-pgru-layer: NormalizeComponent in the recurrence, BatchNorm on the output
    "pg_norm": dict(spec=_pg((_b(norm=True),)), graph="grammar", audio="synth:174:24000"),
    # ... with dropout-proportion given: a DropoutComponent behind each sigmoid (copies in test mode)
    "pg_norm_drop": dict(spec=_pg((_b(norm=True, dropout=True),)), graph="grammar", audio="synth:175:24000"),
    # decay-time=40 at delay 3: the truncation component scales the state by 0.925
    "pg_decay": dict(spec=_pg((_b(scale=0.925),)), graph="grammar", audio="synth:176:24000"),
    # ten cell tiles on eight waves, three r tiles, several k-steps in all three products, several output tiles
    "pg_wide": dict(spec=_pg((_b(cell=160, rec=48, nonrec=48),)), graph="grammar", audio="synth:177:16000"),
    # fast-gru-layer with nine cell tiles on eight waves: the state rows are 144 wide
    "pg_plain_wide": dict(spec=_pg((_plain(cell=144),)), graph="grammar", audio="synth:178:16000"),
    # the largest delay
    "pg_d8": dict(spec=_pg((_b(delay=8),)), graph="grammar", audio="synth:179:24000"),
    # PGRU, tdnn(-3,0,3), norm-PGRU with another shape and a scale, tdnn(-3,0,3); the iVector extractor is on
    "pg_stack": dict(spec=_pg((_b(), _b(after=3, cell=24, rec=8, nonrec=12, norm=True, scale=0.925)), layer_offsets=_TDNN + ((-3, 0, 3),), ivector_dim=10),
                     graph="grammar", audio="synth:180:32000"),
    # an LSTM and an OPGRU block behind the second TDNN layer and a PGRU block behind the third: result matrix 64 + k counts all three
    "pg_mixed": dict(spec=_pg((_b(after=3),), lstm_layers=(dict(after=2, cell=32, rec=8, nonrec=8, delay=3),),
                              gru_layers=(dict(after=2, cell=32, rec=8, nonrec=8, delay=3),)), graph="grammar", audio="synth:181:24000"),
    # --frame-subsampling-factor=3: delay 3 under offsets {-3, 0, 3} is one residue class, delay 2 all three
    "pg_fsf3": dict(spec=_pg(_BASIC), graph="grammar", audio="synth:182:32000", conf_opts={"frame-subsampling-factor": 3}),
    "pg_fsf3_d2": dict(spec=_pg((_b(delay=2),)), graph="grammar", audio="synth:183:32000", conf_opts={"frame-subsampling-factor": 3}),
    "pg_text": dict(spec=_pg(_BASIC, binary=False), graph="grammar", audio="synth:170:24000"),
    # lengths on pg_basic's model: no frame, one frame, two frames (fewer than the delay), one frame more than a chunk of 24, one
    # fewer than two chunks
    "pg_len0": dict(spec=_pg(_BASIC), graph="grammar", audio="synth:184:399"),
    "pg_len1": dict(spec=_pg(_BASIC), graph="grammar", audio="synth:184:400"),
    "pg_len2": dict(spec=_pg(_BASIC), graph="grammar", audio="synth:184:560"),
    "pg_len25": dict(spec=_pg(_BASIC), graph="grammar", audio=f"synth:185:{400 + 24 * 160}"),
    "pg_len47": dict(spec=_pg(_BASIC), graph="grammar", audio=f"synth:186:{400 + 46 * 160}"),
    # no --dither line: the reference's set-up accepts the model, this library refuses it (the rand() position of a recurrent
    # compilation is not replayed)
    "pg_dither_default": dict(spec=_pg(_BASIC, dither=None), graph="grammar", audio="synth:170:24000"),
}
NO_GOLDEN = ("pg_dither_default",)
LENGTHS = ("pg_len0", "pg_len1", "pg_len2", "pg_len25", "pg_len47")


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

class Float64Net(gc.Float64Net):
    """gru_cases.Float64Net with the block around a GruNonlinearityComponent: GruNonlinearityComponent::Propagate
    (nnet-combined-component.cc:1430-1484) between VectorBase::Sigmoid / Tanh, the affine W_y, NormalizePerRow (cu-math.cc:302-310) in
    the norm variant and the truncation component's scale; without a projection (fast-gru-layer) the state is the scaled cell.  A
    chain starts where the block's feed-forward input first exists, with zeros before."""

    def _node(self, name):
        if name not in self.memo and re.match(r"^pgru\d+\.", name):
            b = name.split(".", 1)[0]
            if not (name == f"{b}.y_t" and f"{b}.y_t_tmp" in self.nodes):      # (the norm variant's BatchNorm is an ordinary layer)
                self._pgru_block(b)
                return self.memo[name]
        return super()._node(name)

    def _pgru_block(self, b):
        nodes, comps = self.nodes, self.comps
        m = re.match(r"^Append\((.*), IfDefined\(Offset\((\S+), (-?\d+)\)\)\)$", nodes[f"{b}.z_t_pre"]["input"])
        x_desc, d = m.group(1), -int(m.group(3))
        assert m.group(2) == f"{b}.s_t" and nodes[f"{b}.hpart_t"]["input"] == x_desc
        t0, x = self._desc(x_desc)

        def aff(node):
            f = comps[nodes[node]["component"]][1]
            return f["<LinearParams>"][0].astype(np.float64), f["<BiasParams>"][0].astype(np.float64)

        (Wz, bz), (Wr, br), (Wh, bh) = aff(f"{b}.z_t_pre"), aff(f"{b}.r_t_pre"), aff(f"{b}.hpart_t")
        proj = f"{b}.c_t" in nodes
        norm = f"{b}.y_t_tmp" in nodes
        y_name = f"{b}.y_t_tmp" if norm else f"{b}.y_t"
        w_h = comps[nodes[f"{b}.gru_nonlin_t"]["component"]][1]["<w_h>"][0].astype(np.float64)
        scale = float(np.float32(comps[nodes[f"{b}.s_t"]["component"]][1]["<Scale>"][0]))
        rms = float(np.float32(comps[nodes[f"{b}.s_t_renorm"]["component"]][1]["<TargetRms>"][0])) if norm else 1.0
        in_dim = x.shape[1]
        C, R = w_h.shape
        assert Wz.shape == (C, in_dim + R) and Wr.shape == (R, in_dim + R) and (proj or R == C)
        if proj:
            Wy, by = aff(y_name)
        n = x.shape[0]
        h = np.zeros((n, C)); c = np.zeros((n, C)); s = np.zeros((n, R))
        y = np.zeros((n, Wy.shape[0])) if proj else None
        pre_z, pre_r, hp = x @ Wz[:, :in_dim].T + bz, x @ Wr[:, :in_dim].T + br, x @ Wh.T + bh
        for i in range(n):
            sp = s[i - d] if i >= d else np.zeros(R)
            cp = (c[i - d] if i >= d else np.zeros(C)) if proj else sp
            z = lc._sigmoid(pre_z[i] + Wz[:, in_dim:] @ sp)
            r = lc._sigmoid(pre_r[i] + Wr[:, in_dim:] @ sp)
            h[i] = lc._tanh(hp[i] + w_h @ (r * sp))
            c[i] = h[i] - z * h[i] + z * cp
            if proj:
                y[i] = Wy @ c[i] + by
                v = y[i][:R]
                if norm:
                    v = v * max(gc.K_SQUARED_NORM_FLOOR, float(v @ v) / (R * rms * rms)) ** -0.5
                s[i] = scale * v
            else:
                s[i] = scale * c[i]
        memo = self.memo
        memo[f"{b}.gru_nonlin_t"] = (t0, np.concatenate([h, c], axis=1))
        memo[f"{b}.s_t"] = (t0, s)
        if proj:
            memo[f"{b}.c_t"] = (t0, c)
            memo[y_name] = (t0, y)
        else:
            memo[f"{b}.y_t"] = (t0, c)


def restate(name: str, g=None):
    """(log-likelihoods as the reference lays them out, [block outputs, every frame]) of the case from its golden's input rows, in
    float64."""
    g = load_golden(name) if g is None else g
    spec = cases.case_spec(CASES[name])
    net = Float64Net(spec, *contexts(name))
    iv = g["offline_ivector"][0] if "offline_ivector" in g.files else None
    ll, blocks = net.forward(g["input"], iv)
    return ll[::fsf_of(name)], blocks
