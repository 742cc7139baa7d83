"""TDNN-attention models (RestrictedAttentionComponent: the time-restricted self-attention layers of xconfig/attention.py): the case
table of tests/test_attention_cpu.py, tests/test_gpu_attention.py and tests/gen_attention_golden.py, a restatement of the load-time
planner's choice (csrc/attention_plan.cc) and a float64 numpy restatement of the case networks on top of conv_cases.Float64Net.
Tiny specs as in tests/cases.py (24 phones, 48 pdfs, hidden width 32; clips of 1-2 s); what the reference's two decoder binaries and
rs-dump gave for each is in tests/golden/attention/<case>.npz."""
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests import conv_cases

GOLDEN = cases.GOLDEN / "attention"
NBEST = cases.NBEST

_TDNN = ((0,), (-1, 0, 1), (-3, 0, 3))


def _at(layers, dither=0.0, layer_offsets=_TDNN, **spec):
    s = dict(ivector_dim=0, dither=dither, layer_offsets=layer_offsets, attention_layers=tuple(layers))
    s.update(spec)
    return s


def _a(after=2, heads=2, key_dim=8, value_dim=8, left=2, right=1, stride=1, **kw):
    return dict(after=after, heads=heads, key_dim=key_dim, value_dim=value_dim, left=left, right=right, stride=stride, **kw)


# ------------------------------------------------------------------------------------------ the planner's choice, restated

MAX_LDS_FLOATS, MAX_FRAMES = 64 * 1024 // 4, 128


def plan(layer):
    """(frames, heads per workgroup, head groups, staged rows, pitch, LDS bytes) PlanAttention chooses for a layer dict: as many heads
    as leave a tile of at least four times its context rows (128 frames at most) within 64 KiB of LDS, else one head and the longest
    tile that fits."""
    H, K, V, s = int(layer["heads"]), int(layer["key_dim"]), int(layer["value_dim"]), int(layer["stride"])
    C = int(layer["left"]) + 1 + int(layer["right"])

    def pitch(hg):
        return (hg * (K + V)) | 1

    def frames_for(hg):
        per_frame, fixed = 1 + pitch(hg) + hg * (K + 2 * C), (C - 1) * s * pitch(hg)
        return min(MAX_FRAMES, (MAX_LDS_FLOATS - fixed) // per_frame if MAX_LDS_FLOATS > fixed else 0)

    want = min(MAX_FRAMES, 4 * (C - 1) * s)
    hg = next((h for h in range(H, 1, -1) if frames_for(h) >= want), 1)
    f = frames_for(hg)
    rows = f + (C - 1) * s
    return f, hg, -(-H // hg), rows, pitch(hg), 4 * (f + rows * pitch(hg) + f * hg * (K + 2 * C))


_BASIC = (_a(),)
# one frame more than the frames a workgroup of at_basic's op takes: the clip's last frame is in a second tile whatever the padding
_LEN_N = 400 + plan(_BASIC[0])[0] * 160

CASES = {
    # tdnn(0), tdnn(-1,0,1), attention-relu-renorm-layer H 2 K 8 V 8 L 2 R 1 s 1 with output-context, tdnn(-3,0,3), output
    "at_basic": dict(spec=_at(_BASIC), graph="grammar", audio="synth:120:24000"),
    # one case per layer form: the nodes behind (or, the last, in front of) the attention component
    "at_form_renorm": dict(spec=_at((_a(form="attention-renorm-layer"),)), graph="grammar", audio="synth:221:24000"),
    "at_form_relu_renorm": dict(spec=_at((_a(form="attention-relu-renorm-layer", heads=1),)), graph="grammar", audio="synth:122:24000"),
    "at_form_relu_batchnorm": dict(spec=_at((_a(form="attention-relu-batchnorm-layer"),)), graph="grammar", audio="synth:123:24000"),
    "at_form_relu_renorm_attention": dict(spec=_at((_a(form="relu-renorm-attention-layer"),)), graph="grammar", audio="synth:324:24000"),
    # nothing a multiple of 4, 16 or 64
    "at_odd": dict(spec=_at((_a(heads=3, key_dim=5, value_dim=7, left=3, right=2),)), graph="grammar", audio="synth:125:24000"),
    "at_left_only": dict(spec=_at((_a(left=3, right=0),)), graph="grammar", audio="synth:126:24000"),
    "at_right_only": dict(spec=_at((_a(left=0, right=2),)), graph="grammar", audio="synth:127:24000"),
    "at_stride3": dict(spec=_at((_a(stride=3),)), graph="grammar", audio="synth:128:24000"),
    "at_noctx": dict(spec=_at((_a(output_context=False),)), graph="grammar", audio="synth:129:24000"),
    # an explicit key-scale, not 1 / sqrt(key-dim)
    "at_keyscale": dict(spec=_at((_a(key_scale=0.5),)), graph="grammar", audio="synth:130:24000"),
    # |b| beyond 100: a softmax without the maximum subtracted overflows (the generator asserts max |b| > 100 in the restatement)
    "at_sharp": dict(spec=_at((_a(logit_gain=7.5),)), graph="grammar", audio="synth:431:24000"),
    # a recipe's head shape on a 1 s clip: twelve head groups, several time tiles per utterance
    "at_recipe_head": dict(spec=_at((_a(heads=12, key_dim=40, value_dim=60, left=5, right=2, stride=3),)), graph="grammar", audio="synth:132:16000"),
    # two attention layers of different geometry, a TDNN layer between them
    "at_stack": dict(spec=_at((_a(), _a(after=3, heads=3, key_dim=5, value_dim=7, left=1, right=2, stride=2, form="attention-relu-batchnorm-layer")),
                              layer_offsets=_TDNN + ((-3, 0, 3),)), graph="grammar", audio="synth:133:32000"),
    # --frame-subsampling-factor=3: with stride 3 the op, its affine and everything above run on every third row; with stride 2 the
    # op runs on every third row and reads dense rows
    "at_fsf3": dict(spec=_at((_a(stride=3),)), graph="grammar", audio="synth:134:32000", conf_opts={"frame-subsampling-factor": 3}),
    "at_fsf3_s2": dict(spec=_at((_a(stride=2),)), graph="grammar", audio="synth:135:32000", conf_opts={"frame-subsampling-factor": 3}),
    "at_text": dict(spec=_at(_BASIC, binary=False), graph="grammar", audio="synth:120:24000"),
    # lengths on at_basic's model: no frame, one frame, two frames, one frame more than a workgroup's tile
    "at_len0": dict(spec=_at(_BASIC), graph="grammar", audio="synth:136:399"),
    "at_len1": dict(spec=_at(_BASIC), graph="grammar", audio="synth:236:400"),
    "at_len2": dict(spec=_at(_BASIC), graph="grammar", audio="synth:236:560"),
    "at_lenN": dict(spec=_at(_BASIC), graph="grammar", audio=f"synth:137:{_LEN_N}"),
    # with the iVector branch
    "at_iv": dict(spec=_at(_BASIC, ivector_dim=10), graph="grammar", audio="synth:138:32000"),
    # no --dither line: the rows depend on the rand() position the set-up leaves
    "at_dither_default": dict(spec=_at(_BASIC, dither=None), graph="grammar", audio="synth:139:24000"),
    # zero padding in time (one of the two left inputs is optional): the reference decodes it, this library refuses it at load
    "at_required_subset": dict(spec=_at((_a(left_required=1),)), graph="grammar", audio="synth:140:16000"),
}
NO_GOLDEN = ("at_required_subset",)
LENGTHS = ("at_len0", "at_len1", "at_len2", "at_lenN")
REFUSAL = "num-left-inputs-required 1 is smaller than num-left-inputs 2 (zero padding in time"
MIN_NBEST_GAP = 0.05      # consecutive 5-best totals of every golden are at least this far apart (gen_attention_golden.py checks it)


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


def layers_of(name: str):
    """The case's attention layer dicts in network order, as synth.py names them (attention1, ...): (k, layer)."""
    spec = cases.case_spec(CASES[name])
    order = sorted(range(len(spec.attention_layers)), key=lambda i: (int(spec.attention_layers[i]["after"]), i))
    return [(i + 1, spec.attention_layers[i]) for i in order]


def contexts(name: str):
    """(left, right) context of the case's network: the offsets' sums through every layer."""
    spec = cases.case_spec(CASES[name])
    left = -min(spec.lda_offsets) + sum(-min(o) for o in spec.layer_offsets) + sum(int(l["left"]) * int(l["stride"]) for l in spec.attention_layers)
    right = max(spec.lda_offsets) + sum(max(o) for o in spec.layer_offsets) + sum(int(l["right"]) * int(l["stride"]) for l in spec.attention_layers)
    return left, right


# ------------------------------------------------------------------------------------------ float64 restatement

K_SQUARED_NORM_FLOOR = 2.0 ** -66      # NormalizeComponent::kSquaredNormFloor


class Float64Net(conv_cases.Float64Net):
    """conv_cases.Float64Net with RestrictedAttentionComponent (nnet-attention-component.cc:132-197, attention.cc:97-152: per head
    b = key-scale * <query key, key of row t + (o - L) s> + query context, c = softmax(b), the values of those rows weighted by c, c
    appended with output-context) and NormalizeComponent (cu-math.cc:302-310).  `max_abs_b` is the largest |b| of the real frames."""

    def __init__(self, spec):
        super().__init__(spec)
        self.max_abs_b = 0.0
        for typ, f in self.comps.values():
            if typ == "RestrictedAttentionComponent":
                self.halo += max(f["<NumLeftInputs>"][0], f["<NumRightInputs>"][0]) * f["<TimeStride>"][0]

    def _node(self, name):
        if name not in self.memo and self.nodes[name]["_type"] == "component-node":
            typ, f = self.comps[self.nodes[name]["component"]]
            if typ == "RestrictedAttentionComponent":
                self.memo[name] = self._attention(self._desc(self.nodes[name]["input"]), f)
            elif typ == "NormalizeComponent":
                x = self._desc(self.nodes[name]["input"])
                rms = f["<TargetRms>"][0]
                ss = (x * x).sum(axis=1, keepdims=True) / (x.shape[1] * rms * rms)
                self.memo[name] = x * np.maximum(ss, K_SQUARED_NORM_FLOOR) ** -0.5
        return super()._node(name)

    def _attention(self, x, f):
        H, K, V = f["<NumHeads>"][0], f["<KeyDim>"][0], f["<ValueDim>"][0]
        L, R, s = f["<NumLeftInputs>"][0], f["<NumRightInputs>"][0], f["<TimeStride>"][0]
        assert f["<NumLeftInputsRequired>"][0] == L and f["<NumRightInputsRequired>"][0] == R
        C, scale = L + 1 + R, f["<KeyScale>"][0]
        per_head = 2 * K + V + C
        assert x.shape[1] == H * per_head
        real = slice(self.halo, x.shape[0] - self.halo)
        out = []
        for h in range(H):
            blk = x[:, h * per_head:(h + 1) * per_head]
            key, val, qk, qc = blk[:, :K], blk[:, K:K + V], blk[:, K + V:2 * K + V], blk[:, 2 * K + V:]
            b = np.stack([scale * (qk * self._shift(key, (o - L) * s)).sum(axis=1) + qc[:, o] for o in range(C)], axis=1)
            self.max_abs_b = max(self.max_abs_b, float(np.abs(b[real]).max()) if b[real].size else 0.0)
            e = np.exp(b - b.max(axis=1, keepdims=True))
            c = e / e.sum(axis=1, keepdims=True)
            out.append(sum(c[:, o:o + 1] * self._shift(val, (o - L) * s) for o in range(C)))
            if f["<OutputContext>"][0]:
                out.append(c)
        return np.concatenate(out, axis=1)

    def forward(self, feats, ivector=None):
        """As conv_cases.Float64Net.forward; the second result holds the output rows of every attention component in network order,
        before the nodes behind it."""
        ll, _ = super().forward(feats, ivector)
        T, H = feats.shape[0], self.halo
        names = [n for n, kv in self.nodes.items() if kv["_type"] == "component-node" and self.comps[kv["component"]][0] == "RestrictedAttentionComponent"]
        return ll, [self.memo[n][H:H + T] for n in names]


def restate(name: str, g=None):
    """(log-likelihoods as the reference lays them out, [attention outputs, every frame], max |b|) of the case from its golden's input
    rows, in float64."""
    g = load_golden(name) if g is None else g
    net = Float64Net(cases.case_spec(CASES[name]))
    iv = g["offline_ivector"][0] if "offline_ivector" in (g.files if hasattr(g, "files") else g) else None
    ll, taps = net.forward(g["input"], iv)
    return ll[::fsf_of(name)], taps, net.max_abs_b
