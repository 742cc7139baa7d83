"""CNN-TDNN models (TimeHeightConvolutionComponent front ends): the case table of tests/test_conv_cpu.py, tests/test_gpu_conv.py and
tests/gen_conv_golden.py, and a float64 numpy restatement of the case networks.  The dictionaries are those of tests/cases.py (tiny
specs: 24 phones, 48 pdfs; clips of 1-2 s); what the reference's two decoder binaries and rs-dump gave for each is in
tests/golden/conv/<case>.npz."""
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases

GOLDEN = cases.GOLDEN / "conv"
NBEST = cases.NBEST

R3 = (-1, 0, 1)


def _l(filters, height_out, t=R3, h=R3, **kw):
    return dict(filters=filters, height_out=height_out, time_offsets=t, height_offsets=h, **kw)


def _fb(layers, bins=40, dither=0.0, **spec):
    s = dict(feature_type="fbank", num_mel_bins=bins, ivector_dim=0, dither=dither, conv_layers=tuple(layers), layer_offsets=((0,), (-1, 0, 1)))
    s.update(spec)
    return s


_BASIC = (_l(8, 40), _l(8, 20, sub=2), _l(16, 20, t=(-3, 0, 3)))
_PLUS = ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))

CASES = {
    # K = 9 with padding at both height edges; 40 -> 20 heights by subsampling; time offsets {-3, 0, 3}; then two TDNN layers
    "cv_basic": dict(spec=_fb(_BASIC), graph="grammar", audio="synth:50:24000"),
    # the recipe: MFCC -> idct + batchnorm, iVector -> linear + batchnorm, combine-feature-maps to 6 maps x 40, three
    # conv-relu-batchnorm layers, TDNN-F layers; the reference's default dither, so the set-up's rand() count decides the rows
    "cv_recipe": dict(spec=dict(conv_idct=True, conv_ivector_maps=5, conv_layers=(_l(8, 40), _l(8, 20, sub=2), _l(16, 10, sub=2)),
                                tdnnf=True, bottleneck_dim=16, layer_offsets=((0,), (-1, 0, 1), (-3, 0, 3))),
                      graph="grammar", audio="synth:51:32000"),
    # no padding: height offsets {0, 1, 2}, two heights fewer, K = 27
    "cv_nopad": dict(spec=_fb((_l(3, 40), _l(8, 38, h=(0, 1, 2)))), graph="grammar", audio="synth:52:24000"),
    # nothing a multiple of an MFMA tile edge: 6 -> 20 filters, 13 -> 7 heights
    "cv_odd": dict(spec=_fb((_l(6, 13), _l(20, 7, sub=2)), bins=13), graph="grammar", audio="synth:53:24000"),
    # a plus sign: not a rectangle of offsets; default dither
    "cv_plus": dict(spec=_fb((dict(filters=8, height_out=40, offsets=_PLUS), dict(filters=8, height_out=40, offsets=_PLUS)), dither=None),
                    graph="grammar", audio="synth:54:24000"),
    # a single time offset, and one-sided ones
    "cv_t0": dict(spec=_fb((_l(8, 40, t=(0,)), _l(8, 40, t=(-2, -1, 0)))), graph="grammar", audio="synth:55:24000"),
    # K = 576 and 2560 output columns: several k-steps, several column tiles
    "cv_wide": dict(spec=_fb((_l(64, 40), _l(64, 40)), lda_offsets=(0,)), graph="grammar", audio="synth:56:16000"),
    # four pixel tiles a workgroup (64 input filters leave LDS for three frames of 20 heights): the one-tile-per-wave instantiation
    "cv_m1": dict(spec=_fb((_l(64, 40), _l(16, 20, sub=2)), lda_offsets=(0,)), graph="grammar", audio="synth:60:16000"),
    # --frame-subsampling-factor=3 over time offsets {-3, 0, 3}: both convolutions and everything above them are read at t = 0 mod 3
    # only and run on every third row; the first one reads the (dense) input rows at {-1, 0, 1} around those
    "cv_fsf3": dict(spec=_fb((_l(8, 40), _l(8, 20, t=(-3, 0, 3), sub=2)), lda_offsets=(0,), layer_offsets=((0,), (-3, 0, 3))), graph="grammar",
                    audio="synth:57:32000", conf_opts={"frame-subsampling-factor": 3}),
    "cv_text": dict(spec=_fb(_BASIC, binary=False), graph="grammar", audio="synth:50:24000"),
    # a clip too short for one frame, and exactly one frame (the model of cv_basic)
    "cv_len0": dict(spec=_fb(_BASIC), graph="grammar", audio="synth:58:399"),
    "cv_len1": dict(spec=_fb(_BASIC), graph="grammar", audio="synth:58:400"),
    # zero padding in time (the middle offset alone is required): the reference decodes it, this library refuses it at load
    "cv_required_subset": dict(spec=_fb((_l(8, 40, required_time_offsets=(0,)),)), graph="grammar", audio="synth:59:16000"),
}
NO_GOLDEN = ("cv_required_subset",)
REFUSAL = "its required time offsets are a proper subset of its time offsets"


def model_key(name: str):
    """Cases with the same key decode with one model and one graph."""
    c = CASES[name]
    return repr((sorted(c["spec"].items(), key=str), c["graph"], c.get("conf_opts"), c.get("opts")))


def build_case_files(name: str, root: Path):
    """(model_dir, graph_dir, wav, pcm) of the case under `root`."""
    return cases.build_case_files(CASES[name], root)


def load_golden(name: str):
    return np.load(GOLDEN / f"{name}.npz")


def conv_geometry(name: str):
    """Per convolution layer of the case: (filters_in, filters_out, height_in, height_out, sub, offsets, distinct time offsets)."""
    spec = cases.case_spec(CASES[name])
    height, filters = spec.feat_dim, 1 + spec.conv_ivector_maps
    out = []
    for layer in spec.conv_layers:
        offs = synth.conv_layer_offsets(layer)
        f_out, h_out = int(layer["filters"]), int(layer["height_out"])
        out.append((filters, f_out, height, h_out, int(layer.get("sub", 1)), offs, sorted({t for t, _ in offs})))
        filters, height = f_out, h_out
    return out


# ------------------------------------------------------------------------------------------ float64 restatement

class _Recorder(synth.KaldiWriter):
    """Takes what a component's writer function writes and keeps it as {token: value}: the network's parameters as synth.py made
    them, without reading a file back."""

    def __init__(self):
        super().__init__(True)
        self.fields, self._tok = {}, None

    def token(self, tok):
        self._tok = tok
        self.fields.setdefault(tok, [])
        return self

    def _put(self, v):
        self.fields[self._tok].append(v)
        return self

    def nl(self): return self
    def i32(self, v): return self._put(int(v))
    def f32(self, v): return self._put(float(np.float32(v)))
    def f64(self, v): return self._put(float(v))
    def boolean(self, v): return self._put(bool(v))
    def int_vector(self, v): return self._put([int(x) for x in v])
    def int_pair_vector(self, v): return self._put([(int(a), int(b)) for a, b in v])
    def vector(self, v, double=False): return self._put(np.asarray(v, np.float32 if not double else np.float64).astype(np.float64))
    def matrix(self, m, double=False): return self._put(np.asarray(m, np.float32 if not double else np.float64).astype(np.float64))


class Float64Net:
    """The case's network in float64, straight from its definition (convolution.h:90-208; nnet-simple-component.cc for the rest):
    rows are frames on a time axis padded by edge replication of the INPUT, as the reference's decodable pads it."""

    def __init__(self, spec: synth.ModelSpec):
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
        self.halo = 2
        for kv in self.nodes.values():
            o = [abs(int(x)) for x in re.findall(r"Offset\([^()]*?,\s*(-?\d+)\s*[,)]", kv.get("input", ""))]
            node_max = max(o) if o else 0
            if kv["_type"] == "component-node":
                typ, f = self.comps[kv["component"]]
                if typ == "TdnnComponent":
                    node_max += max(abs(x) for x in f["<TimeOffsets>"][0])
                if typ == "TimeHeightConvolutionComponent":
                    node_max += max(abs(t) for t, _ in f["<Offsets>"][0])
            self.halo += node_max

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
    def _shift(a, o):
        return a if o == 0 else a[np.clip(np.arange(a.shape[0]) + o, 0, a.shape[0] - 1)]

    def _desc(self, s):
        s = s.strip()
        m = re.match(r"^(\w+)\((.*)\)$", s, re.S)
        if m and m.group(1) in ("Append", "Sum", "Offset", "Scale", "ReplaceIndex"):
            fn, args = m.group(1), self._split(m.group(2))
            if fn == "Append":
                return np.concatenate([self._desc(a) for a in args], axis=1)
            if fn == "Sum":
                return sum(self._desc(a) for a in args)
            if fn == "Offset":
                return self._shift(self._desc(args[0]), int(args[1]))
            if fn == "Scale":
                return float(np.float32(float(args[0]))) * self._desc(args[1])
            return self._desc(args[0])      # ReplaceIndex(ivector, t, 0): the iVector rows are constant over t already
        return self._node(s)

    def _node(self, name):
        if name in self.memo:
            return self.memo[name]
        kv = self.nodes[name]
        if kv["_type"] == "output-node":
            out = self._desc(kv["input"])
        else:
            typ, f = self.comps[kv["component"]]
            x = self._desc(kv["input"])
            if typ in ("NaturalGradientAffineComponent", "AffineComponent", "FixedAffineComponent"):
                out = x @ f["<LinearParams>"][0].T + f["<BiasParams>"][0][None, :]
            elif typ == "LinearComponent":
                out = x @ f["<Params>"][0].T
            elif typ == "TdnnComponent":
                W, b, d = f["<LinearParams>"][0], f["<BiasParams>"][0], x.shape[1]
                out = np.zeros((x.shape[0], W.shape[0])) + (b[None, :] if b.size else 0.0)
                for i, o in enumerate(f["<TimeOffsets>"][0]):
                    out = out + self._shift(x, o) @ W[:, i * d:(i + 1) * d].T
            elif typ == "TimeHeightConvolutionComponent":
                out = self._conv(x, f)
            elif typ == "PermuteComponent":
                out = x[:, f["<ColumnMap>"][0]]
            elif typ == "RectifiedLinearComponent":
                out = np.maximum(x, 0.0)
            elif typ == "BatchNormComponent":
                mean, var = f["<StatsMean>"][0], f["<StatsVar>"][0]
                scale = f["<TargetRms>"][0] / np.sqrt(var + f["<Epsilon>"][0])
                reps = f["<Dim>"][0] // len(mean)
                out = x * np.tile(scale, reps)[None, :] + np.tile(-mean * scale, reps)[None, :]
            elif typ in ("NoOpComponent", "GeneralDropoutComponent"):
                out = x
            else:
                raise ValueError(typ)
        self.memo[name] = out
        return out

    @staticmethod
    def _conv(x, f):
        fi, fo = f["<NumFiltersIn>"][0], f["<NumFiltersOut>"][0]
        hi, ho, sub = f["<HeightIn>"][0], f["<HeightOut>"][0], f["<HeightSubsampleOut>"][0]
        W, b = f["<LinearParams>"][0], f["<BiasParams>"][0]
        assert x.shape[1] == hi * fi and W.shape == (fo, len(f["<Offsets>"][0]) * fi)
        xin = x.reshape(x.shape[0], hi, fi)
        out = np.zeros((x.shape[0], ho, fo)) + b[None, None, :]
        for o, (dt, dh) in enumerate(f["<Offsets>"][0]):
            xs = Float64Net._shift(xin, dt)
            Wo = W[:, o * fi:(o + 1) * fi]
            for h in range(ho):
                h_in = h * sub + dh
                if 0 <= h_in < hi:
                    out[:, h, :] += xs[:, h_in, :] @ Wo.T
        return out.reshape(x.shape[0], ho * fo)

    def forward(self, feats, ivector=None):
        """feats: T x C golden `input` rows; ivector: None or the one row every frame sees.  Returns (T x pdfs log-likelihoods,
        [per convolution layer, T x dim: the layer's output after its ReLU and BatchNorm, what the fused device op stores])."""
        T, H = feats.shape[0], self.halo
        idx = np.clip(np.arange(-H, T + H), 0, T - 1)
        self.memo = {"input": feats[idx].astype(np.float64)}
        if ivector is not None:
            self.memo["ivector"] = np.tile(np.asarray(ivector, np.float64).reshape(1, -1), (T + 2 * H, 1))
        out = self._node("output")[H:H + T]
        layers = [self.memo[f"cnn{i}.batchnorm"][H:H + T] for i in range(1, 100) if f"cnn{i}.batchnorm" in self.memo]
        return out, layers


def restate(name: str, g=None):
    """(log-likelihoods as the reference lays them out, [conv layer outputs, every frame]) of the case from its golden's input rows,
    in float64."""
    g = load_golden(name) if g is None else g
    spec = cases.case_spec(CASES[name])
    net = Float64Net(spec)
    iv = g["offline_ivector"][0] if "offline_ivector" in g.files else None
    ll, conv = net.forward(g["input"], iv)
    fsf = int(CASES[name].get("conf_opts", {}).get("frame-subsampling-factor", 1))
    return ll[::fsf], conv
