"""TDNN-LSTM models whose cell is spelled out as separate components (nnet3's lstmp-layer / lstmp-batchnorm-layer / lstm-layer: four
NaturalGradientAffineComponents, three NaturalGradientPerElementScaleComponent peepholes, Sigmoid / Tanh nodes, three
ElementwiseProductComponents, two truncation components): the case table of tests/test_lstmp_cpu.py, tests/test_gpu_lstmp.py and
tests/gen_lstmp_golden.py, and a float64 numpy restatement of the case networks.  The dictionaries are those of tests/cases.py (tiny
specs: 24 phones, 48 pdfs, hidden width 32; clips of 1-2 s); what the reference's two decoder binaries and rs-dump gave for each is
in tests/golden/lstmp/<case>.npz."""
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests import lstm_cases as lc

GOLDEN = cases.GOLDEN / "lstmp"
NBEST = cases.NBEST

_TDNN = ((0,), (-1, 0, 1), (-3, 0, 3))


def _lp(layers, dither=0.0, layer_offsets=_TDNN, **spec):
    s = dict(ivector_dim=0, dither=dither, layer_offsets=layer_offsets, lstm_layers=tuple(layers))
    s.update(spec)
    return s


def _b(after=2, cell=32, rec=8, nonrec=8, delay=3, form="composed", **kw):
    return dict(after=after, cell=cell, rec=rec, nonrec=nonrec, delay=delay, form=form, **kw)


_BASIC = (_b(),)

CASES = {
    # tdnn(0), tdnn(-1,0,1), lstmp-layer C=32 R=8 P=8 delay 3, tdnn(-3,0,3), output
    "lp_basic": dict(spec=_lp(_BASIC), graph="grammar", audio="synth:70:24000"),
    # nothing a multiple of 16, R != P, delay 1
    "lp_odd": dict(spec=_lp((_b(cell=20, rec=6, nonrec=10, delay=1),)), graph="grammar", audio="synth:71:24000"),
    # lstm-layer: no projection, the state is scale_r m, the layers above read m_t
    "lp_noproj": dict(spec=_lp((_b(cell=24, rec=0, nonrec=0, delay=2),)), graph="grammar", audio="synth:72:24000"),
    # more than one column tile in every product and several k-steps
    "lp_wide": dict(spec=_lp((_b(cell=160, rec=48, nonrec=48),)), graph="grammar", audio="synth:100:16000"),
    # decay-time=40 at delay 3: both truncation components scale by 0.925 -- the cell BEFORE the output gate's peephole and Tanh,
    # which is where the composed order parts from the fast block's
    "lp_decay": dict(spec=_lp((_b(scale=0.925),)), graph="grammar", audio="synth:74:24000"),
    # the two components' scales are read separately (xconfig always writes one value: through synth only)
    "lp_scales": dict(spec=_lp((_b(scale_c=0.9, scale_r=0.8),)), graph="grammar", audio="synth:73:24000"),
    # dropout-proportion given: the shared DropoutComponent behind i, f and o, a copy in test mode
    "lp_drop": dict(spec=_lp((_b(dropout=True),)), graph="grammar", audio="synth:75:24000"),
    # older models: ClipGradientComponent truncation nodes
    "lp_clipgrad": dict(spec=_lp((_b(clipgrad=True),)), graph="grammar", audio="synth:78:24000"),
    # two blocks with a tdnn(-3,0,3) between and above, the second lstmp-batchnorm-layer; the iVector extractor is on
    "lp_stack": dict(spec=_lp((_b(), _b(after=3, cell=24, rec=8, nonrec=16, batchnorm=True)), layer_offsets=_TDNN + ((-3, 0, 3),), ivector_dim=10),
                     graph="grammar", audio="synth:83:32000"),
    # a fast-lstmp block and a composed one in one network: block numbering, result matrix 64 + k
    "lp_mixed": dict(spec=_lp((_b(form="fast"), _b(after=3, cell=24, rec=8, nonrec=16)), layer_offsets=_TDNN + ((-3, 0, 3),)),
                     graph="grammar", audio="synth:84:32000"),
    # --frame-subsampling-factor=3: delay 3 under offsets {-3, 0, 3} is one residue class, delay 2 all three
    "lp_fsf3": dict(spec=_lp(_BASIC), graph="grammar", audio="synth:77:32000", conf_opts={"frame-subsampling-factor": 3}),
    "lp_fsf3_d2": dict(spec=_lp((_b(delay=2),)), graph="grammar", audio="synth:100:32000", conf_opts={"frame-subsampling-factor": 3}),
    "lp_d8": dict(spec=_lp((_b(delay=8),)), graph="grammar", audio="synth:85:24000"),
    "lp_text": dict(spec=_lp(_BASIC, binary=False), graph="grammar", audio="synth:70:24000"),
    # lengths on lp_basic's model: no frame, one frame, two frames (fewer than the delay), one frame more than a chunk of 24, one
    # fewer than two chunks
    "lp_len0": dict(spec=_lp(_BASIC), graph="grammar", audio="synth:79:399"),
    "lp_len1": dict(spec=_lp(_BASIC), graph="grammar", audio="synth:100:400"),
    "lp_len2": dict(spec=_lp(_BASIC), graph="grammar", audio="synth:100:560"),
    "lp_len25": dict(spec=_lp(_BASIC), graph="grammar", audio=f"synth:100:{400 + 24 * 160}"),
    "lp_len47": dict(spec=_lp(_BASIC), graph="grammar", audio=f"synth:81:{400 + 46 * 160}"),
    # no --dither line: the reference's set-up accepts the model, this library refuses it (the rand() position of a recurrent
    # compilation is not replayed)
    "lp_dither_default": dict(spec=_lp(_BASIC, dither=None), graph="grammar", audio="synth:70:24000"),
}
NO_GOLDEN = ("lp_dither_default",)
LENGTHS = ("lp_len0", "lp_len1", "lp_len2", "lp_len25", "lp_len47")


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
    """Per recurrent block of the case, in network order: (block number as synth names it, composed, input dim, cell, recurrent,
    non-recurrent, delay, scale_c, scale_r, dropout)."""
    spec = cases.case_spec(CASES[name])
    out = []
    for after in range(1, len(spec.layer_offsets) + 1):
        in_dim = spec.hidden_dim
        for k, layer in enumerate(spec.lstm_layers, start=1):
            if int(layer["after"]) != after:
                continue
            C, R, P, out_dim = synth.lstm_layer_dims(layer)
            scale = float(layer.get("scale", 1.0))
            out.append((k, layer.get("form", "fast") == "composed", in_dim, C, R, P, int(layer.get("delay", 3)),
                        float(layer.get("scale_c", scale)), float(layer.get("scale_r", scale)), int(bool(layer.get("dropout", False)))))
            in_dim = out_dim
    return out


def contexts(name: str):
    """(left, right) context of the case's network: the offsets' sums through the feed-forward layers (ComputeSimpleNnetContext
    ignores the optional recurrent dependency)."""
    spec = cases.case_spec(CASES[name])
    return (-min(spec.lda_offsets) + sum(-min(o) for o in spec.layer_offsets), max(spec.lda_offsets) + sum(max(o) for o in spec.layer_offsets))


# ------------------------------------------------------------------------------------------ float64 restatement

_sigmoid, _tanh = lc._sigmoid, lc._tanh      # (VectorBase::Sigmoid / Tanh, kaldi-vector.cc:899-951, are the same functions)

_BLOCK_NODES = ("c_t", "h_t", "g1_t", "g_t", "c1_t", "c2_t", "m_t", "rp_t", "r_t_preclip", "r_t") + tuple(
    f"{g}{s}" for g in "ifo" for s in ("1_t", "2_t", "_t", "_t_predrop"))


class Float64Net(lc.Float64Net):
    """lstm_cases.Float64Net (the time axis, the rows that exist, the feed-forward nodes, the fast block) with the composed block:
    the recurrence of xconfig/lstm.py's XconfigLstmpLayer / XconfigLstmLayer, node by node."""

    # True: the output gate and Tanh read the cell before its truncation scale, as LstmNonlinearityComponent orders it (the tests
    # use it to show that a case tells the two orders apart)
    fast_order = False

    def _node(self, name):
        if name not in self.memo and "." in name:
            b, leaf = name.rsplit(".", 1)
            if leaf in _BLOCK_NODES and f"{b}.c1_t" in self.nodes:
                self._composed(b)
                return self.memo[name]
        return super()._node(name)

    def _composed(self, b):
        nodes, comps = self.nodes, self.comps
        m = re.match(r"^Append\((.*), IfDefined\(Offset\((\S+), (-?\d+)\)\)\)$", nodes[f"{b}.i1_t"]["input"])
        x_desc, d = m.group(1), -int(m.group(3))
        assert m.group(2) == f"{b}.r_t"
        proj = f"{b}.rp_t" in nodes
        t0, x = self._desc(x_desc)
        in_dim = x.shape[1]
        Wx, Wr, bias, peep = {}, {}, {}, {}
        for g, comp in (("i", "W_i.xr"), ("f", "W_f.xr"), ("g", "W_c.xr"), ("o", "W_o.xr")):
            f = comps[f"{b}.{comp}"][1]
            W = f["<LinearParams>"][0]
            Wx[g], Wr[g], bias[g] = W[:, :in_dim], W[:, in_dim:], f["<BiasParams>"][0]
        for g in "ifo":
            peep[g] = comps[f"{b}.w_{g}.c"][1]["<Params>"][0].astype(np.float64)
        C = peep["i"].shape[0]

        def scale_of(comp):
            f = comps[comp][1]
            return float(np.float32(f["<Scale>"][0])) if "<Scale>" in f else 1.0      # (a ClipGradientComponent has none)
        scale_c, scale_r = scale_of(f"{b}.c"), scale_of(f"{b}.r")
        if proj:
            fr = comps[f"{b}.W_rp.m"][1]
            Wrp, brp = fr["<LinearParams>"][0], fr["<BiasParams>"][0]
        pre = {g: x @ Wx[g].T + bias[g][None, :] for g in "ifgo"}
        n = x.shape[0]
        rec_dim = Wr["i"].shape[1]
        sc = np.zeros((n, C)); mm = np.zeros((n, C)); sr = np.zeros((n, rec_dim))
        rp = np.zeros((n, Wrp.shape[0])) if proj else None
        for i in range(n):
            cp = sc[i - d] if i >= d else np.zeros(C)
            rprev = sr[i - d] if i >= d else np.zeros(rec_dim)
            a = {g: pre[g][i] + Wr[g] @ rprev for g in "ifgo"}
            i_t = _sigmoid(a["i"] + peep["i"] * cp)
            f_t = _sigmoid(a["f"] + peep["f"] * cp)
            g_t = _tanh(a["g"])
            sc[i] = scale_c * (f_t * cp + i_t * g_t)
            cur = sc[i] / scale_c if self.fast_order else sc[i]
            o_t = _sigmoid(a["o"] + peep["o"] * cur)      # (the peephole on the current, already scaled cell)
            mm[i] = o_t * _tanh(cur)
            if proj:
                rp[i] = Wrp @ mm[i] + brp
                sr[i] = scale_r * rp[i][:rec_dim]
            else:
                sr[i] = scale_r * mm[i]
        memo = self.memo
        memo[f"{b}.c_t"] = (t0, sc)
        memo[f"{b}.m_t"] = (t0, mm)
        memo[f"{b}.r_t"] = (t0, sr)
        if proj:
            memo[f"{b}.rp_t"] = (t0, rp)
            memo[f"{b}.r_t_preclip"] = (t0, rp[:, :rec_dim])

    def forward(self, feats, ivector=None):
        """As lstm_cases.Float64Net.forward; the block rows are rp_t / m_t of a composed block, rp / m of a fast one."""
        T, L, H = feats.shape[0], self.L, self.R + 2
        idx = np.clip(np.arange(-L, T + H), 0, T - 1)
        self.memo = {"input": (-L, feats[idx].astype(np.float64))}
        if ivector is not None:
            self.memo["ivector"] = (-L, np.tile(np.asarray(ivector, np.float64).reshape(1, -1), (T + L + H, 1)))
        t0, out = self._node("output")
        assert t0 <= 0 and out.shape[0] + t0 >= T, (t0, out.shape)
        blocks = []
        for k in range(1, 100):
            key = next((f"lstm{k}.{leaf}" for leaf in ("rp_t", "rp", "m_t", "m") if f"lstm{k}.{leaf}" in self.nodes), None)
            if key is None or key not in self.memo:
                break
            bt0, rows = self.memo[key]
            blocks.append(rows[-bt0:-bt0 + T])
        return out[-t0:-t0 + T], blocks


def restate(name: str, g=None):
    """(log-likelihoods as the reference lays them out, [block outputs, every frame]) of the case from its golden's input rows, in
    float64."""
    g = load_golden(name) if g is None else g
    spec = cases.case_spec(CASES[name])
    net = Float64Net(spec, *contexts(name))
    iv = g["offline_ivector"][0] if "offline_ivector" in g.files else None
    ll, blocks = net.forward(g["input"], iv)
    return ll[::fsf_of(name)], blocks
