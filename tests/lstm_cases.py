"""TDNN-LSTM models (nnet3's fast-lstmp-layer / fast-lstm-layer: LstmNonlinearityComponent, BackpropTruncationComponent,
DropoutMaskComponent): the case table of tests/test_lstm_cpu.py, tests/test_gpu_lstm.py and tests/gen_lstm_golden.py, and a float64
numpy restatement of the case networks.  The dictionaries are those of tests/cases.py (tiny specs: 24 phones, 48 pdfs, hidden width
32; clips of 1-2 s); what the reference's two decoder binaries and rs-dump gave for each is in tests/golden/lstm/<case>.npz."""
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests.conv_cases import _Recorder

GOLDEN = cases.GOLDEN / "lstm"
NBEST = cases.NBEST

_TDNN = ((0,), (-1, 0, 1), (-3, 0, 3))


def _ls(layers, dither=0.0, layer_offsets=_TDNN, **spec):
    s = dict(ivector_dim=0, dither=dither, layer_offsets=layer_offsets, lstm_layers=tuple(layers))
    s.update(spec)
    return s


def _b(after=2, cell=32, rec=8, nonrec=8, delay=3, **kw):
    return dict(after=after, cell=cell, rec=rec, nonrec=nonrec, delay=delay, **kw)


_BASIC = (_b(),)

CASES = {
    # tdnn(0), tdnn(-1,0,1), LSTMP C=32 R=8 P=8 delay 3, tdnn(-3,0,3), output
    "ls_basic": dict(spec=_ls(_BASIC), graph="grammar", audio="synth:70:24000"),
    # nothing a multiple of 16, R != P, delay 1
    "ls_odd": dict(spec=_ls((_b(cell=20, rec=6, nonrec=10, delay=1),)), graph="grammar", audio="synth:71:24000"),
    # fast-lstm-layer: no projection, the state goes through cm_trunc, the layers above read m
    "ls_noproj": dict(spec=_ls((_b(cell=24, rec=0, nonrec=0, delay=2),)), graph="grammar", audio="synth:72:24000"),
    # two blocks with a tdnn(-3,0,3) between and above, the second with BatchNorm on rp; the iVector extractor is on
    "ls_stack": dict(spec=_ls((_b(), _b(after=3, cell=24, rec=8, nonrec=16, batchnorm=True)), layer_offsets=_TDNN + ((-3, 0, 3),), ivector_dim=10),
                     graph="grammar", audio="synth:83:32000"),
    # decay-time=40 at delay 3: the truncation component scales the state by 0.925
    "ls_decay": dict(spec=_ls((_b(scale=0.925),)), graph="grammar", audio="synth:74:24000"),
    # use-dropout=true: the nonlinearity's input carries the three columns of a DropoutMaskComponent node
    "ls_dropmask": dict(spec=_ls((_b(dropout=True),)), graph="grammar", audio="synth:75:24000"),
    # more than one column tile in every product and several k-steps
    "ls_wide": dict(spec=_ls((_b(cell=160, rec=48, nonrec=48),)), graph="grammar", audio="synth:76:16000"),
    # --frame-subsampling-factor=3: delay 3 under offsets {-3, 0, 3} is one residue class, delay 2 all three
    "ls_fsf3": dict(spec=_ls(_BASIC), graph="grammar", audio="synth:77:32000", conf_opts={"frame-subsampling-factor": 3}),
    "ls_fsf3_d2": dict(spec=_ls((_b(delay=2),)), graph="grammar", audio="synth:88:32000", conf_opts={"frame-subsampling-factor": 3}),
    "ls_text": dict(spec=_ls(_BASIC, binary=False), graph="grammar", audio="synth:70:24000"),
    # lengths on ls_basic's model: no frame, one frame, two frames (fewer than the delay), one frame more than a chunk of 24, one
    # fewer than two chunks
    "ls_len0": dict(spec=_ls(_BASIC), graph="grammar", audio="synth:79:399"),
    "ls_len1": dict(spec=_ls(_BASIC), graph="grammar", audio="synth:79:400"),
    "ls_len2": dict(spec=_ls(_BASIC), graph="grammar", audio="synth:79:560"),
    "ls_len25": dict(spec=_ls(_BASIC), graph="grammar", audio=f"synth:80:{400 + 24 * 160}"),
    "ls_len47": dict(spec=_ls(_BASIC), graph="grammar", audio=f"synth:81:{400 + 46 * 160}"),
    # no --dither line: the reference's set-up accepts the model, this library refuses it (the rand() position of a recurrent
    # compilation is not replayed)
    "ls_dither_default": dict(spec=_ls(_BASIC, dither=None), graph="grammar", audio="synth:70:24000"),
}
NO_GOLDEN = ("ls_dither_default",)
LENGTHS = ("ls_len0", "ls_len1", "ls_len2", "ls_len25", "ls_len47")


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
    """Per recurrent block of the case, in network order: (input dim, cell, recurrent, non-recurrent, delay, scale, dropout mask)."""
    spec = cases.case_spec(CASES[name])
    out = []
    for after in range(1, len(spec.layer_offsets) + 1):
        in_dim = spec.hidden_dim
        for layer in spec.lstm_layers:
            if int(layer["after"]) != after:
                continue
            C, R, P, out_dim = synth.lstm_layer_dims(layer)
            out.append((in_dim, C, R, P, int(layer.get("delay", 3)), float(layer.get("scale", 1.0)), int(bool(layer.get("dropout", False)))))
            in_dim = out_dim
    return out


def contexts(name: str):
    """(left, right) context of the case's network: the offsets' sums through the feed-forward layers (ComputeSimpleNnetContext
    ignores the optional recurrent dependency)."""
    spec = cases.case_spec(CASES[name])
    return (-min(spec.lda_offsets) + sum(-min(o) for o in spec.layer_offsets), max(spec.lda_offsets) + sum(max(o) for o in spec.layer_offsets))


# ------------------------------------------------------------------------------------------ float64 restatement

def _sigmoid(a):
    # ScalarSigmoid (cu-math.cc:422-431), both branches
    e = np.exp(-np.abs(a))
    return np.where(a > 0, 1.0 / (1.0 + e), e / (e + 1.0))


def _tanh(a):
    # ScalarTanh (cu-math.cc:433-442)
    e = np.exp(-np.abs(a))
    return np.where(a > 0, -1.0 + 2.0 / (1.0 + e * e), 1.0 - 2.0 / (1.0 + e * e))


class Float64Net:
    """The case's network in float64, straight from its definition.  Time axis: t in [-left_context, T + halo), the INPUT replicated
    at both edges as the reference's decodable pads it.  Which rows exist is the computation graph builder's decision, restated: a
    feed-forward node is computable at t when all its inputs are, the input itself from t = -left_context on; a recurrent block's
    chain t, t - d, ... starts at the earliest t' of its residue class at which the block's feed-forward input is computable, and
    IfDefined supplies zeros before that.  Rows to the right of T - 1 continue the recurrence on the replicated input."""

    def __init__(self, spec: synth.ModelSpec, left_context: int, right_context: int):
        cfg, comps = synth.build_nnet(spec, np.random.default_rng(spec.seed))
        self.comps = {}
        for name, fn in comps:
            r = _Recorder()
            fn(r)
            typ = next(iter(r.fields))[1:-1]
            self.comps[name] = (typ, r.fields)
        self.nodes = {}
        for ln in cfg:
            first, rest = ln.split(None, 1)
            keys = [(m.start(1), m.end()) for m in re.finditer(r"(?:^|\s)([\w-]+)=", rest)]
            kv = {rest[ks:ve - 1]: rest[ve:(keys[i + 1][0] if i + 1 < len(keys) else len(rest))].strip() for i, (ks, ve) in enumerate(keys)}
            kv["_type"] = first
            self.nodes[kv["name"]] = kv
        self.L, self.R = left_context, right_context

    # A value is (first t at which the node is computable, its rows from that t on)

    @staticmethod
    def _split(s):
        out, depth, cur = [], 0, ""
        for ch in s:
            depth += (ch == "(") - (ch == ")")
            if ch == "," and depth == 0:
                out.append(cur.strip())
                cur = ""
            else:
                cur += ch
        return out + [cur.strip()]

    @staticmethod
    def _align(vals):
        """Common time axis of several values: from the latest first-t on, all to the shortest right end."""
        t0 = max(v[0] for v in vals)
        rows = [v[1][t0 - v[0]:] for v in vals]
        n = min(r.shape[0] for r in rows)
        return t0, [r[:n] for r in rows]

    def _desc(self, s):
        s = s.strip()
        m = re.match(r"^(\w+)\((.*)\)$", s, re.S)
        if m and m.group(1) in ("Append", "Sum", "Offset", "Scale", "ReplaceIndex"):
            fn, args = m.group(1), self._split(m.group(2))
            if fn == "Append":
                t0, rows = self._align([self._desc(a) for a in args])
                return t0, np.concatenate(rows, axis=1)
            if fn == "Sum":
                t0, rows = self._align([self._desc(a) for a in args])
                return t0, sum(rows)
            if fn == "Offset":
                t0, a = self._desc(args[0])
                o = int(args[1])
                # x[t + o]: row i of the result is t = t0 - o + i
                return t0 - o, a
            if fn == "Scale":
                t0, a = self._desc(args[1])
                return t0, float(np.float32(float(args[0]))) * a
            return self._desc(args[0])      # ReplaceIndex(ivector, t, 0): the iVector rows are constant over t already
        return self._node(s)

    def _node(self, name):
        if name in self.memo:
            return self.memo[name]
        kv = self.nodes[name]
        if kv["_type"] == "dim-range-node":
            src = kv["input-node"]
            if src.endswith(".lstm_nonlin") or src.endswith("_trunc") or (src.endswith(".rp") and src[:-3] + ".W_all" in self.nodes):
                self._block(src.rsplit(".", 1)[0])
                return self.memo[name]
            t0, a = self._node(src)
            o, d = int(kv["dim-offset"]), int(kv["dim"])
            out = (t0, a[:, o:o + d])
        elif kv["_type"] == "output-node":
            out = self._desc(kv["input"])
        else:
            typ, f = self.comps[kv["component"]]
            if name.endswith((".W_all", ".lstm_nonlin", ".cr_trunc", ".cm_trunc")) or (name.endswith(".rp") and name[:-3] + ".W_all" in self.nodes):
                self._block(name.rsplit(".", 1)[0])
                return self.memo[name]
            t0, x = self._desc(kv["input"])
            if typ in ("NaturalGradientAffineComponent", "AffineComponent", "FixedAffineComponent"):
                y = x @ f["<LinearParams>"][0].T + f["<BiasParams>"][0][None, :]
            elif typ == "RectifiedLinearComponent":
                y = np.maximum(x, 0.0)
            elif typ == "BatchNormComponent":
                mean, var = f["<StatsMean>"][0], f["<StatsVar>"][0]
                scale = f["<TargetRms>"][0] / np.sqrt(var + f["<Epsilon>"][0])
                y = x * scale[None, :] + (-mean * scale)[None, :]
            elif typ == "BackpropTruncationComponent":
                y = float(np.float32(f["<Scale>"][0])) * x
            else:
                raise ValueError(typ)
            out = (t0, y)
        self.memo[name] = out
        return out

    def _block(self, b):
        """One recurrent block (xconfig/lstm.py:1120-1198 / 706-753; CpuComputeLstmNonlinearity, cu-math.cc:445-486)."""
        nodes, comps = self.nodes, self.comps
        w_all = nodes[f"{b}.W_all"]
        m = re.match(r"^Append\((.*), IfDefined\(Offset\((\S+), (-?\d+)\)\)\)$", w_all["input"])
        x_desc, d = m.group(1), -int(m.group(3))
        proj = f"{b}.rp" in nodes
        t0, x = self._desc(x_desc)
        fa = comps[w_all["component"]][1]
        W, bias = fa["<LinearParams>"][0], fa["<BiasParams>"][0]
        params = comps[nodes[f"{b}.lstm_nonlin"]["component"]][1]["<Params>"][0]
        C = params.shape[1]
        trunc = f"{b}.cr_trunc" if proj else f"{b}.cm_trunc"
        scale = float(np.float32(comps[nodes[trunc]["component"]][1]["<Scale>"][0]))
        if proj:
            fr = comps[nodes[f"{b}.rp"]["component"]][1]
            Wrp, brp = fr["<LinearParams>"][0], fr["<BiasParams>"][0]
        in_dim = x.shape[1]
        Wx, Wr = W[:, :in_dim], W[:, in_dim:]
        pre = x @ Wx.T + bias[None, :]
        n = x.shape[0]
        rec_dim = Wr.shape[1]
        c = np.zeros((n, C)); mm = np.zeros((n, C)); sc = np.zeros((n, C)); sr = np.zeros((n, rec_dim))
        rp = np.zeros((n, Wrp.shape[0])) if proj else None
        for i in range(n):
            cp = sc[i - d] if i >= d else np.zeros(C)
            rprev = sr[i - d] if i >= d else np.zeros(rec_dim)
            g = pre[i] + Wr @ rprev
            i_t = _sigmoid(g[:C] + params[0] * cp)
            f_t = _sigmoid(g[C:2 * C] + params[1] * cp)
            c_t = f_t * cp + i_t * _tanh(g[2 * C:3 * C])
            o_t = _sigmoid(g[3 * C:] + params[2] * c_t)
            m_t = o_t * _tanh(c_t)
            c[i], mm[i] = c_t, m_t
            if proj:
                rp[i] = Wrp @ m_t + brp
                sr[i] = scale * rp[i][:rec_dim]
            else:
                sr[i] = scale * m_t
            sc[i] = scale * c_t
        memo = self.memo
        memo[f"{b}.W_all"] = (t0, pre)      # (the feed-forward part only; nothing outside the block reads it)
        memo[f"{b}.lstm_nonlin"] = (t0, np.concatenate([c, mm], axis=1))
        memo[f"{b}.m"] = (t0, mm)
        memo[f"{b}.c_trunc"] = (t0, sc)
        if proj:
            memo[f"{b}.c"] = (t0, c)
            memo[f"{b}.rp"] = (t0, rp)
            memo[f"{b}.r"] = (t0, rp[:, :rec_dim])
            memo[f"{b}.cr_trunc"] = (t0, np.concatenate([sc, sr], axis=1))
            memo[f"{b}.r_trunc"] = (t0, sr)
        else:
            memo[f"{b}.cm_trunc"] = (t0, np.concatenate([sc, sr], axis=1))
            memo[f"{b}.m_trunc"] = (t0, sr)

    def forward(self, feats, ivector=None):
        """feats: T x C golden `input` rows; ivector: None or the one row every frame sees.  Returns (T x pdfs log-likelihoods,
        [per recurrent block, T x dim: the rows the layers above read -- rp, or m without a projection])."""
        T, L, H = feats.shape[0], self.L, self.R + 2
        idx = np.clip(np.arange(-L, T + H), 0, T - 1)
        self.memo = {"input": (-L, feats[idx].astype(np.float64))}
        if ivector is not None:
            self.memo["ivector"] = (-L, np.tile(np.asarray(ivector, np.float64).reshape(1, -1), (T + L + H, 1)))
        t0, out = self._node("output")
        assert t0 <= 0 and out.shape[0] + t0 >= T, (t0, out.shape)
        blocks = []
        for k in range(1, 100):
            key = f"lstm{k}.rp" if f"lstm{k}.rp" in self.nodes else f"lstm{k}.m"
            if key not in self.memo:
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
