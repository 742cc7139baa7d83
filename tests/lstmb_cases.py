"""TDNN-LSTM models whose cell sits behind a bottleneck (nnet3's lstmb-layer: the LinearComponents W_all_a and W_all_b, the
ScaleAndOffsetComponent W_all_b_so, an LstmNonlinearityComponent, one BackpropTruncationComponent, Scale() on the recurrent input):
the case table of tests/test_lstmb_cpu.py, tests/test_gpu_lstmb.py and tests/gen_lstmb_golden.py, and a float64 numpy restatement of
the case networks.  The dictionaries are those of tests/cases.py (tiny specs: 24 phones, 48 pdfs, hidden width 32; clips of 1-2 s);
what the reference's two decoder binaries and rs-dump gave for each is in tests/golden/lstmb/<case>.npz."""
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests import lstmp_cases as lp

GOLDEN = cases.GOLDEN / "lstmb"
NBEST = cases.NBEST

_TDNN = ((0,), (-1, 0, 1), (-3, 0, 3))
_T33 = ((-3, 0, 3),)


def _lb(layers, dither=0.0, layer_offsets=_TDNN, **spec):
    s = dict(ivector_dim=0, dither=dither, layer_offsets=layer_offsets, lstm_layers=tuple(layers))
    s.update(spec)
    return s


def _b(after=2, cell=32, bottleneck=16, delay=3, **kw):
    return dict(after=after, cell=cell, bottleneck=bottleneck, delay=delay, **kw)


_BASIC = (_b(),)
# scales that EnsureNonzero moves (0, +5e-5, -5e-5) between ordinary ones, repeated along the 4 cell entries (7 and 128 are coprime:
# every gate has some of each); W_all_b is 200 times its usual size and the ordinary scales are small to match, so that a moved
# scale, 1e-4 against 0 or 5e-5, changes a gate's input by about 0.01
_SO_SCALES = (0.0, 5e-5, -5e-5, 0.004, -0.006, 0.005, 0.003)
_SO_OFFSETS = (0.3, -0.2, 0.1, -0.4, 0.25)

CASES = {
    # tdnn(0), tdnn(-1,0,1), lstmb-layer C=32 B=16 delay 3, tdnn(-3,0,3), output
    "lb_basic": dict(spec=_lb(_BASIC), graph="grammar", audio="synth:70:24000"),
    # nothing a multiple of 16, one partial tile in each phase, delay 1
    "lb_odd": dict(spec=_lb((_b(cell=20, bottleneck=12, delay=1),)), graph="grammar", audio="synth:71:24000"),
    # 10 cell tiles and 9 bottleneck tiles: more items than waves in both phases, several k blocks
    "lb_wide": dict(spec=_lb((_b(cell=160, bottleneck=144),)), graph="grammar", audio="synth:76:16000"),
    # the bottleneck wider than the cell
    "lb_bgtc": dict(spec=_lb((_b(cell=24, bottleneck=40),)), graph="grammar", audio="synth:72:24000"),
    # decay-time=40 at delay 3: the truncation component scales the state by 0.925
    "lb_decay": dict(spec=_lb((_b(scale=0.925),)), graph="grammar", audio="synth:74:24000"),
    # self-scale=0.5 on top of it: sm = 0.5 (0.925 m), two roundings
    "lb_selfscale": dict(spec=_lb((_b(scale=0.925, self_scale=0.5),)), graph="grammar", audio="synth:73:24000"),
    # EnsureNonzero
    "lb_so": dict(spec=_lb((_b(so_scales=_SO_SCALES, so_offsets=_SO_OFFSETS, wb_gain=200.0),)), graph="grammar", audio="synth:75:24000"),
    # two blocks with a tdnn(-3,0,3) between and above; the iVector extractor is on
    "lb_stack": dict(spec=_lb((_b(), _b(after=3, cell=24, bottleneck=8, self_scale=0.75)), layer_offsets=_TDNN + _T33, ivector_dim=10),
                     graph="grammar", audio="synth:83:32000"),
    # a fast-lstmp block, a composed block and an lstmb block in one network: block numbering, result matrix 64 + k
    "lb_mixed": dict(spec=_lb((dict(after=2, cell=32, rec=8, nonrec=8, delay=3), dict(after=3, cell=24, rec=8, nonrec=16, delay=3, form="composed"),
                               _b(after=4, cell=24, bottleneck=16)), layer_offsets=_TDNN + _T33 + _T33),
                     graph="grammar", audio="synth:84:32000"),
    # --frame-subsampling-factor=3: delay 3 under offsets {-3, 0, 3} is one residue class, delay 2 all three
    "lb_fsf3": dict(spec=_lb(_BASIC), graph="grammar", audio="synth:77:32000", conf_opts={"frame-subsampling-factor": 3}),
    "lb_fsf3_d2": dict(spec=_lb((_b(delay=2),)), graph="grammar", audio="synth:88:32000", conf_opts={"frame-subsampling-factor": 3}),
    "lb_d8": dict(spec=_lb((_b(delay=8),)), graph="grammar", audio="synth:85:24000"),
    "lb_text": dict(spec=_lb(_BASIC, binary=False), graph="grammar", audio="synth:70:24000"),
    # lengths on lb_basic's model: no frame, one frame, two frames (fewer than the delay), one frame more than a chunk of 24, one
    # fewer than two chunks
    "lb_len0": dict(spec=_lb(_BASIC), graph="grammar", audio="synth:79:399"),
    "lb_len1": dict(spec=_lb(_BASIC), graph="grammar", audio="synth:79:400"),
    "lb_len2": dict(spec=_lb(_BASIC), graph="grammar", audio="synth:100:560"),
    "lb_len25": dict(spec=_lb(_BASIC), graph="grammar", audio=f"synth:100:{400 + 24 * 160}"),
    "lb_len47": dict(spec=_lb(_BASIC), graph="grammar", audio=f"synth:81:{400 + 46 * 160}"),
    # no recurrent block: a ScaleAndOffsetComponent in its block form, dim 32 over 8-long vectors, between two TDNN layers
    "lb_so_ff": dict(spec=_lb((), scale_offset_layers=(dict(after=2, block=8),)), graph="grammar", audio="synth:86:24000"),
    # no --dither line: the reference's set-up accepts the model, this library refuses it (the rand() position of a recurrent
    # compilation is not replayed)
    "lb_dither_default": dict(spec=_lb(_BASIC, dither=None), graph="grammar", audio="synth:70:24000"),
}
NO_GOLDEN = ("lb_dither_default",)
LENGTHS = ("lb_len0", "lb_len1", "lb_len2", "lb_len25", "lb_len47")


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
    """Per recurrent block of the case, in network order: (block number as synth names it, kind -- "lstm", "lstmp" or "lstmb" --,
    input dim, cell, bottleneck (0: none), delay, scale, self_scale)."""
    spec = cases.case_spec(CASES[name])
    out = []
    for after in range(1, len(spec.layer_offsets) + 1):
        in_dim = spec.hidden_dim
        for k, layer in enumerate(spec.lstm_layers, start=1):
            if int(layer["after"]) != after:
                continue
            C, R, P, out_dim = synth.lstm_layer_dims(layer)
            kind = "lstmb" if "bottleneck" in layer else "lstmp" if layer.get("form", "fast") == "composed" else "lstm"
            out.append((k, kind, in_dim, C, int(layer.get("bottleneck", 0)), int(layer.get("delay", 3)), float(layer.get("scale", 1.0)),
                        float(layer.get("self_scale", 1.0))))
            in_dim = out_dim
    return out


def contexts(name: str):
    """(left, right) context of the case's network: the offsets' sums through the feed-forward layers (ComputeSimpleNnetContext
    ignores the optional recurrent dependency)."""
    spec = cases.case_spec(CASES[name])
    return (-min(spec.lda_offsets) + sum(-min(o) for o in spec.layer_offsets), max(spec.lda_offsets) + sum(max(o) for o in spec.layer_offsets))


# ------------------------------------------------------------------------------------------ float64 restatement

_sigmoid, _tanh = lp._sigmoid, lp._tanh
_EPSILON = float(np.float32(1e-4))      # ScaleAndOffsetComponent::Epsilon()


def ensure_nonzero(s):
    """cu::EnsureNonzero (cu-math.cc:226-238) on a float32 vector, in float64."""
    s = np.asarray(s, np.float64)
    return np.where((s <= -_EPSILON) | (s >= _EPSILON), s, np.where(s >= 0.0, _EPSILON, -_EPSILON))


class Float64Net(lp.Float64Net):
    """lstmp_cases.Float64Net (the time axis, the rows that exist, the feed-forward nodes, the fast and the composed block) with the
    block behind a bottleneck, the recurrence of xconfig/lstm.py's XconfigLstmbLayer node by node, and ScaleAndOffsetComponent as a
    feed-forward node."""

    # the tests turn these off to show that a case tells the difference
    apply_scale_offset = True
    apply_ensure_nonzero = True

    def _scale_offset(self, f, x):
        if not self.apply_scale_offset:
            return x
        s, o = f["<Scales>"][0], f["<Offsets>"][0].astype(np.float64)
        s = ensure_nonzero(s) if self.apply_ensure_nonzero else s.astype(np.float64)
        rep = x.shape[1] // s.shape[0]      # (the block form: the vectors repeat along the row)
        return x * np.tile(s, rep)[None, :] + np.tile(o, rep)[None, :]

    def _node(self, name):
        kv = self.nodes.get(name)
        if name not in self.memo and kv is not None and kv["_type"] == "component-node" and not name.endswith(".W_all_b_so"):
            typ, f = self.comps[kv["component"]]
            if typ == "ScaleAndOffsetComponent":
                t0, x = self._desc(kv["input"])
                self.memo[name] = (t0, self._scale_offset(f, x))
        if name not in self.memo and name.endswith((".W_all_a", ".W_all_b", ".W_all_b_so")):
            self._block(name.rsplit(".", 1)[0])
        return super()._node(name)

    def _block(self, b):
        if f"{b}.W_all_a" not in self.nodes:
            return super()._block(b)
        nodes, comps = self.nodes, self.comps
        m = re.match(r"^Append\((.*), IfDefined\(Offset\((.+), (-?\d+)\)\)\)$", nodes[f"{b}.W_all_a"]["input"])
        x_desc, rec, d = m.group(1), m.group(2), -int(m.group(3))
        ms = re.match(r"^Scale\(([^,]+), (\S+)\)$", rec)
        self_scale = float(np.float32(float(ms.group(1)))) if ms else 1.0
        assert (ms.group(2) if ms else rec) == f"{b}.m_trunc"
        t0, x = self._desc(x_desc)
        in_dim = x.shape[1]
        Wa = comps[f"{b}.W_all_a"][1]["<Params>"][0].astype(np.float64)
        Wb = comps[f"{b}.W_all_b"][1]["<Params>"][0].astype(np.float64)
        so = comps[f"{b}.W_all_b_so"][1]
        params = comps[f"{b}.lstm_nonlin"][1]["<Params>"][0]
        C = params.shape[1]
        scale = float(np.float32(comps[f"{b}.cm_trunc"][1]["<Scale>"][0]))
        Wax, Wam = Wa[:, :in_dim], Wa[:, in_dim:]
        assert Wam.shape[1] == C and Wb.shape == (4 * C, Wa.shape[0])
        pre = x @ Wax.T
        n = x.shape[0]
        c = np.zeros((n, C)); mm = np.zeros((n, C)); sc = np.zeros((n, C)); sm = np.zeros((n, C))
        for i in range(n):
            cp = sc[i - d] if i >= d else np.zeros(C)
            mp = sm[i - d] if i >= d else np.zeros(C)
            g = self._scale_offset(so, (Wb @ (pre[i] + Wam @ mp))[None, :])[0]
            i_t = _sigmoid(g[:C] + params[0] * cp)
            f_t = _sigmoid(g[C:2 * C] + params[1] * cp)
            c_t = f_t * cp + i_t * _tanh(g[2 * C:3 * C])
            o_t = _sigmoid(g[3 * C:] + params[2] * c_t)
            m_t = o_t * _tanh(c_t)
            c[i], mm[i] = c_t, m_t
            sc[i] = scale * c_t
            sm[i] = self_scale * (scale * m_t)
        memo = self.memo
        memo[f"{b}.W_all_a"] = memo[f"{b}.W_all_b"] = memo[f"{b}.W_all_b_so"] = (t0, pre)      # (nothing outside the block reads them)
        memo[f"{b}.lstm_nonlin"] = (t0, np.concatenate([c, mm], axis=1))
        memo[f"{b}.m"] = (t0, mm)
        memo[f"{b}.cm_trunc"] = (t0, np.concatenate([sc, scale * mm], axis=1))
        memo[f"{b}.c_trunc"] = (t0, sc)
        memo[f"{b}.m_trunc"] = (t0, scale * mm)


def restate(name: str, g=None, **switches):
    """(log-likelihoods as the reference lays them out, [block outputs, every frame]) of the case from its golden's input rows, in
    float64.  switches: Float64Net's apply_scale_offset / apply_ensure_nonzero."""
    g = load_golden(name) if g is None else g
    spec = cases.case_spec(CASES[name])
    net = Float64Net(spec, *contexts(name))
    for k, v in switches.items():
        assert hasattr(Float64Net, k), k
        setattr(net, k, v)
    iv = g["offline_ivector"][0] if "offline_ivector" in g.files else None
    ll, blocks = net.forward(g["input"], iv)
    return ll[::fsf_of(name)], blocks
