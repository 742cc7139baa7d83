"""Feed-forward nnet3 graph forms -- relu-renorm TDNNs, row-wise components on column ranges, chains of elementwise stages behind the
layer GEMMs and on their own, the scale / offset components, Sum() descriptors of up to eight terms, sixteen-part Appends, row-wise
components behind a Sum() or in front of further elementwise nodes: the case table of tests/test_ff_cpu.py, tests/test_gpu_ff.py and
tests/gen_ff_golden.py, the networks (written by hand: components through synth's KaldiWriter, one config line per node), a float64
numpy restatement of them, and a restatement of how Nnet::Compile lowers them to ops.  Extractor, tree, graph and transition model are
those of tests/cases.py's tiny spec (16 Gaussians, iVector dim 10, dither 0); clips of 1.5 s.  What the reference's two decoder
binaries and rs-dump gave for each case is in tests/golden/ff/<case>.npz."""
import math
import re
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases
from tests.conv_cases import _Recorder

GOLDEN = cases.GOLDEN / "ff"
NBEST = cases.NBEST

SPLICE = "Append(Offset(input, -1), input, Offset(input, 1), ReplaceIndex(ivector, t, 0))"
_EPSILON = float(np.float32(1e-4))                  # ScaleAndOffsetComponent::Epsilon()
_NORM_FLOOR = 1.3552527156068805425e-20             # kSquaredNormFloor (nnet-normalize-component.h: 2^-66)


# ------------------------------------------------------------------------------------------ component writers

def _w_fixed_scale(w, scales):
    # nnet-simple-component.cc:3717-3722
    w.token("<FixedScaleComponent>").token("<Scales>").vector(scales).token("</FixedScaleComponent>")


def _w_fixed_bias(w, bias):
    # nnet-simple-component.cc:3793-3798
    w.token("<FixedBiasComponent>").token("<Bias>").vector(bias).token("</FixedBiasComponent>")


def _w_per_element_scale(w, scales):
    # nnet-simple-component.cc:2091-2096, behind WriteUpdatableCommon
    synth._updatable_open(w, "PerElementScaleComponent")
    w.token("<Params>").vector(scales).token("</PerElementScaleComponent>")


def _w_per_element_offset(w, offsets):
    # nnet-simple-component.cc:2297-2306, behind WriteUpdatableCommon
    synth._updatable_open(w, "PerElementOffsetComponent")
    w.token("<Offsets>").vector(offsets).token("<Dim>").i32(offsets.shape[0]).token("<UseNaturalGradient>").boolean(True)
    w.token("</PerElementOffsetComponent>")


# ------------------------------------------------------------------------------------------ the networks

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


def _call(s):
    """("Append", [args]) of "Append(...)"; (None, None) of a node name."""
    m = re.match(r"^(\w+)\((.*)\)$", s.strip(), re.S)
    if m and m.group(1) in ("Append", "Sum", "Offset", "Scale", "ReplaceIndex", "IfDefined"):
        return m.group(1), _split(m.group(2))
    return None, None


def app(src, offsets):
    return synth._append_desc(src, offsets)


class Net:
    """Config lines and component writers of one network, node by node; every method returns the node's name."""

    def __init__(self, spec, seed):
        self.rng = np.random.default_rng(seed)
        self.C, self.D, self.P = spec.feat_dim, spec.ivector_dim, spec.num_pdfs
        self.cfg = [f"input-node name=input dim={self.C}", f"input-node name=ivector dim={self.D}"]
        self.comps = []
        self.dims = {"input": self.C, "ivector": self.D}

    def dim_of(self, desc):
        fn, args = _call(desc)
        if fn == "Append":
            return sum(self.dim_of(a) for a in args)
        if fn == "Scale":
            return self.dim_of(args[1])
        if fn is not None:
            return self.dim_of(args[0])
        return self.dims[desc.strip()]

    def _add(self, name, writer, desc, dim):
        self.comps.append((name, writer))
        self.cfg.append(f"component-node name={name} component={name} input={desc}")
        self.dims[name] = dim
        return name

    def _randw(self, o, i):
        return (self.rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def affine(self, name, desc, out, bias_shift=0.0, gain=1.0):
        k = self.dim_of(desc)
        W = self._randw(out, k) * np.float32(gain)
        if desc == SPLICE:      # (the columns that see raw MFCCs, magnitude 10-80, are scaled down as a trained LDA whitens)
            W[:, :3 * self.C] *= np.float32(0.04)
        b = (self.rng.standard_normal(out) * 0.1 * gain + bias_shift).astype(np.float32)
        return self._add(name, lambda w: synth._w_affine(w, "NaturalGradientAffineComponent", W, b), desc, out)

    def tdnn(self, name, desc, offsets, out):
        k = self.dim_of(desc) * len(offsets)
        W, b = self._randw(out, k), (self.rng.standard_normal(out) * 0.1).astype(np.float32)
        return self._add(name, lambda w: synth._w_tdnn(w, offsets, W, b), desc, out)

    def output_affine(self, name, desc):
        k = self.dim_of(desc)
        W, b = self._randw(self.P, k) * np.float32(0.25), (self.rng.standard_normal(self.P) * 0.5).astype(np.float32)
        return self._add(name, lambda w: synth._w_affine(w, "NaturalGradientAffineComponent", W, b), desc, self.P)

    def relu(self, name, desc):
        d = self.dim_of(desc)
        return self._add(name, lambda w: synth._w_nonlinear(w, "RectifiedLinearComponent", d), desc, d)

    def log_softmax(self, name, desc):
        d = self.dim_of(desc)
        return self._add(name, lambda w: synth._w_nonlinear(w, "LogSoftmaxComponent", d), desc, d)

    def norm(self, name, desc, target_rms=1.0, add_log_stddev=False, block_dim=None):
        d = self.dim_of(desc)
        block = d if block_dim is None else block_dim

        def write(w):      # nnet-normalize-component.cc:98-111 (<BlockDim> only where it differs from the dim)
            w.token("<NormalizeComponent>").token("<InputDim>").i32(d)
            if block != d:
                w.token("<BlockDim>").i32(block)
            w.token("<TargetRms>").f32(target_rms).token("<AddLogStddev>").boolean(add_log_stddev).token("</NormalizeComponent>")
        return self._add(name, write, desc, d + (d // block if add_log_stddev else 0))

    def noop(self, name, desc):
        d = self.dim_of(desc)
        return self._add(name, lambda w: synth._w_noop(w, d), desc, d)

    def bn(self, name, desc):
        d = self.dim_of(desc)
        mean, var = (0.4 + 0.1 * self.rng.standard_normal(d)).astype(np.float32), self.rng.uniform(0.1, 0.5, d).astype(np.float32)
        return self._add(name, lambda w: synth._w_batchnorm(w, mean, var), desc, d)

    def trunc(self, name, desc, scale):
        d = self.dim_of(desc)
        return self._add(name, lambda w: synth._w_backprop_truncation(w, d, scale, 3), desc, d)

    def _signed(self, d, lo=0.5, hi=1.5):
        return (self.rng.uniform(lo, hi, d) * self.rng.choice([-1.0, 1.0], d)).astype(np.float32)

    def fixed_scale(self, name, desc):
        d = self.dim_of(desc)
        s = self._signed(d)
        return self._add(name, lambda w: _w_fixed_scale(w, s), desc, d)

    def pes(self, name, desc):
        d = self.dim_of(desc)
        s = self._signed(d)
        return self._add(name, lambda w: _w_per_element_scale(w, s), desc, d)

    def ngpes(self, name, desc):
        d = self.dim_of(desc)
        s = self._signed(d)
        return self._add(name, lambda w: synth._w_ng_per_element_scale(w, s), desc, d)

    def fixed_bias(self, name, desc):
        d = self.dim_of(desc)
        b = (self.rng.standard_normal(d) * 0.3).astype(np.float32)
        return self._add(name, lambda w: _w_fixed_bias(w, b), desc, d)

    def peo(self, name, desc):
        d = self.dim_of(desc)
        b = (self.rng.standard_normal(d) * 0.3).astype(np.float32)
        return self._add(name, lambda w: _w_per_element_offset(w, b), desc, d)

    def so(self, name, desc, block=None, scales=None):
        d = self.dim_of(desc)
        block = d if block is None else block
        s = self._signed(block) if scales is None else np.asarray(scales, np.float32)
        o = (self.rng.standard_normal(block) * 0.3).astype(np.float32)
        assert s.shape[0] == block and d % block == 0
        return self._add(name, lambda w: synth._w_scale_and_offset(w, s, o, d), desc, d)

    def dim_range(self, name, src, offset, dim):
        self.cfg.append(f"dim-range-node name={name} input-node={src} dim-offset={offset} dim={dim}")
        self.dims[name] = dim
        return name

    def output(self, desc):
        self.cfg.append(f"output-node name=output input={desc} objective=linear")


def _net_renorm(n, width, floor=False):
    """Kaldi's pre-batchnorm stock recipe, relu-renorm-layer: affine, relu, NormalizeComponent; target-rms 1.0, 0.5, 1.0.  floor: the
    second layer's bias is about -50, its relu rows are all zero (the third layer then reads the first as well)."""
    x = n.norm("tdnn1.renorm", n.relu("tdnn1.relu", n.affine("tdnn1.affine", SPLICE, width)), 1.0)
    y = n.affine("tdnn2.affine", app(x, (-1, 0, 1)), width, bias_shift=-50.0 if floor else 0.0)
    y = n.norm("tdnn2.renorm", n.relu("tdnn2.relu", y), 0.5)
    d3 = app(y, (-3, 0, 3))
    if floor:
        d3 = d3[:-1] + f", {x})"
    z = n.norm("tdnn3.renorm", n.relu("tdnn3.relu", n.affine("tdnn3.affine", d3, width)), 1.0)
    n.output(n.output_affine("output.affine", z))


def _net_range(n):
    """NormalizeComponent over columns [40, 88) of a 128-wide layer, columns [88, 128) read by the next affine directly; a
    LogSoftmaxComponent over the pdfs."""
    a = n.relu("tdnn1.relu", n.affine("tdnn1.affine", SPLICE, 128))
    mid = n.norm("mid.renorm", n.dim_range("tdnn1.mid", a, 40, 48), 1.0)
    rest = n.dim_range("tdnn1.rest", a, 88, 40)
    b = n.affine("tdnn2.affine", f"Append(Offset({mid}, -1), {mid}, Offset({mid}, 1), {rest})", 64)
    b = n.bn("tdnn2.batchnorm", n.relu("tdnn2.relu", b))
    n.output(n.log_softmax("output.log-softmax", n.output_affine("output.affine", b)))


def _chain(n, p, x, which):
    """One of the four stage chains behind node x; the nodes are named <p>.<stage>."""
    if which == 0:      # batchnorm, relu: the reverse of the relu-batchnorm pattern
        return n.relu(f"{p}.relu", n.bn(f"{p}.batchnorm", x))
    if which == 1:
        return n.bn(f"{p}.batchnorm", n.fixed_bias(f"{p}.bias", n.pes(f"{p}.scale", n.relu(f"{p}.relu", x))))
    if which == 2:
        return n.trunc(f"{p}.trunc", n.relu(f"{p}.relu", x), 0.5)
    x = n.bn(f"{p}.batchnorm", n.fixed_bias(f"{p}.bias", n.pes(f"{p}.scale", n.relu(f"{p}.relu", x))))
    return n.so(f"{p}.so", n.trunc(f"{p}.trunc", x, 0.5))      # six stages


def _net_chains(n, width, rot):
    """Four layers, offsets (0,), (-1,0,1), (-3,0,3), (0,), each with one of the four stage chains behind its affine (rot: which
    layer gets which), the six-stage chain once more as an elementwise op of its own (its source has two readers)."""
    x = _chain(n, "tdnn1", n.affine("tdnn1.affine", SPLICE, width), rot % 4)
    x = _chain(n, "tdnn2", n.affine("tdnn2.affine", app(x, (-1, 0, 1)), width), (rot + 1) % 4)
    x = _chain(n, "tdnn3", n.affine("tdnn3.affine", app(x, (-3, 0, 3)), width), (rot + 2) % 4)
    x = _chain(n, "tdnn4", n.affine("tdnn4.affine", x, width), (rot + 3) % 4)
    e = _chain(n, "six", x, 3)
    n.output(n.output_affine("output.affine", f"Append({x}, {e})"))


# |scale| < 1e-4 of both signs and a zero between ordinary ones (EnsureNonzero moves them to +-1e-4).  The affines in front are
# 5000 times their usual size and the ordinary scales small to match, so that a moved scale changes its column by about 0.5.
_SO_SCALES = (0.0, 2e-5, -2e-5, 1.6e-4, -2.4e-4, 2e-4, 1.2e-4, -2e-4)
_SO_KINDS = ("fixed_scale", "pes", "ngpes", "fixed_bias", "peo", "so")


def _net_so(n):
    """Each scale / offset component twice: behind a layer that the next affine reads as well (it cannot fuse: an elementwise op),
    and behind a relu with no other reader (fused into the layer GEMM)."""
    prev = n.relu("tdnn0.relu", n.affine("tdnn0.affine", SPLICE, 40))
    for i, kind in enumerate(_SO_KINDS):
        mk = (lambda name, d: n.so(name, d, block=8, scales=_SO_SCALES)) if kind == "so" else getattr(n, kind)
        gain = 5000.0 if kind == "so" else 1.0
        # (behind a relu: CollapseModel folds a FixedScaleComponent that reads an affine into a copy of that affine)
        a = n.relu(f"{kind}.a_relu", n.affine(f"{kind}.a", app(prev, (-1, 0, 1) if i % 2 else (0,)), 40, gain=gain))
        u = mk(f"{kind}.unfused", a)
        # (the second reader: the next affine; behind the large affine, through a plain ScaleAndOffset that brings it back to order 1)
        r = n.so(f"{kind}.a_down", a, scales=np.full(40, 2e-4)) if kind == "so" else a
        b = n.relu(f"{kind}.b_relu", n.affine(f"{kind}.b", f"Append({u}, {r})", 40, gain=gain))
        prev = mk(f"{kind}.fused", b)
    n.output(n.output_affine("output.affine", prev))


_SUM3 = "Sum(Offset(a.relu, -2), Scale(0.5, b.relu), Offset(Scale(-1.5, c.relu), 3))"
_SUM2 = "Sum(Scale(0.66, a.relu), Offset(b.relu, 1))"
# (the reference gives a node one scale throughout a Sum: BinarySumDescriptor::GetScaleForNode, nnet-descriptor.cc:411-438)
_SUM8 = ("Sum(a.relu, Offset(a.relu, -1), Scale(0.5, b.relu), Offset(Scale(0.5, b.relu), 2), Scale(-0.25, c.relu), "
         "Scale(-0.25, Offset(c.relu, -3)), sum3.noop, Offset(Scale(0.5, sum2.noop), 1))")


def _net_sums(n):
    """Sums of 2, 3 and 8 terms with mixed Offset and Scale feeding a NoOp and a ReLU; the 3-term sum and a lone Scale() as parts of
    an affine's Append; a TDNN-F style residual; a 2-term sum as a part of a TdnnComponent's input; an output-node over a Sum."""
    for k in "abc":
        n.relu(f"{k}.relu", n.affine(f"{k}.affine", SPLICE, 48))
    n.noop("sum3.noop", _SUM3)
    n.relu("sum3.relu", _SUM3)
    n.noop("sum2.noop", _SUM2)
    n.relu("sum8.relu", _SUM8)
    d = n.relu("d.relu", n.affine("d.affine", f"Append(sum3.noop, sum3.relu, sum8.relu, {_SUM3}, Scale(0.5, a.relu))", 48))
    d2 = n.relu("d2.relu", n.affine("d2.affine", d, 48))
    res = n.noop("res.noop", f"Sum(Scale(0.66, {d}), {d2})")
    e = n.relu("e.relu", n.tdnn("e.tdnn", f"Append({res}, Sum(Offset(a.relu, -1), Scale(2.0, {res})))", (-1, 0, 1), 48))
    ha, hb = n.output_affine("head_a", e), n.output_affine("head_b", f"Append({e}, {d})")
    n.output(f"Sum({ha}, Scale(0.5, {hb}))")


def _segs_parts(extra=False):
    parts = [f"Offset(a.batchnorm, {o})" if o else "a.batchnorm" for o in (-3, -2, -1, 0, 1, 2, 3)]
    parts += ["a.lo", "Offset(a.lo, -1)", "a.hi", "Offset(a.hi, 2)", "ReplaceIndex(ivector, t, 0)", "Offset(input, -1)", "input",
              "Offset(input, 1)", "Offset(a.hi, -4)"]
    return parts + (["Offset(a.lo, 4)"] if extra else [])


def _net_segs(n, extra=False):
    """An affine over an Append of 16 parts (offsets, two dim-ranges, the iVector, the input itself); the output-node names a
    dim-range-node that covers all of the last affine: it is an alias of that buffer."""
    a = n.bn("a.batchnorm", n.relu("a.relu", n.affine("a.affine", SPLICE, 64)))
    n.dim_range("a.lo", a, 0, 24)
    n.dim_range("a.hi", a, 24, 40)
    b = n.relu("b.relu", n.affine("b.affine", "Append(" + ", ".join(_segs_parts(extra)) + ")", 64))
    o = n.output_affine("output.affine", b)
    n.output(n.dim_range("output.all", o, 0, n.P))


def _net_rowwise(n, form):
    """A row-wise component in the positions the lowering used to fuse: relu or batchnorm behind a NormalizeComponent, a
    NormalizeComponent or LogSoftmaxComponent over a Sum() or a Scale()."""
    a = n.affine("tdnn1.affine", SPLICE, 64)
    if form in ("relu", "bn"):
        x = n.norm("tdnn1.renorm", a, 1.0)
        x = n.relu("tdnn1.relu", x) if form == "relu" else n.bn("tdnn1.batchnorm", x)
    else:
        a = n.relu("tdnn1.relu", a)
        b = n.relu("side.relu", n.affine("side.affine", SPLICE, 64))
        desc = {"sum": f"Sum({a}, {b})", "sum_off": f"Sum(Offset({a}, -1), Scale(2, {b}))", "lsm_scale": a}[form]
        x = n.norm("tdnn1.renorm", desc, 0.5) if form != "lsm_scale" else n.noop("tdnn1.noop", f"Sum({a}, Scale(0.5, {b}))")
    y = n.bn("tdnn2.batchnorm", n.relu("tdnn2.relu", n.affine("tdnn2.affine", app(x, (-3, 0, 3)), 64)))
    o = n.output_affine("output.affine", y)
    n.output(n.log_softmax("output.log-softmax", f"Scale(0.5, {o})") if form == "lsm_scale" else o)


def _net_ifdef(n):
    """IfDefined(Offset(x, -2)) outside any cycle, as a part of an affine's Append.  The reference decodes it: the optional term
    adds nothing to the network's context (the golden's is 1, 1), and the rows of x it then cannot compute, t - 2 < 0, count as
    zeros -- frames 0 and 1 differ from a plain Offset(x, -2), every other frame agrees.  The library has no optional inputs in the
    feed-forward path and refuses the descriptor at load."""
    x = n.relu("tdnn1.relu", n.affine("tdnn1.affine", SPLICE, 64))
    y = n.relu("tdnn2.relu", n.affine("tdnn2.affine", f"Append({x}, IfDefined(Offset({x}, -2)))", 64))
    n.output(n.output_affine("output.affine", y))


# what the library refuses at load, each with the words its message has to carry: the node and the reason
REFUSED = {
    "append_elt": ["Append() feeding a non-affine component", "node bad.relu"],
    "ivector_elt": ["elementwise component over the iVector input is not supported", "node bad.relu"],
    "add_log_stddev": ["NormalizeComponent add-log-stddev=true is not supported", "node bad.renorm"],
    "block_dim": ["NormalizeComponent with block-dim is not supported", "node bad.renorm"],
    "terms9": ["bad.noop", "sums too many terms"],
    "stages7": ["tdnn1.affine+tdnn1.relu+s1+s2+s3+s4+s5+s6", "too many fused stages"],
    "segs17": ["b.affine", "too many input segments"],
    "const": ["Const() in the input of node bad.noop is supported only as"],
    "ifdef": ["IfDefined() in the input of node tdnn2.affine (over tdnn1.relu) is supported only as the recurrent connection"],
}


def _net_refused(n, what):
    if what == "segs17":
        return _net_segs(n, extra=True)
    if what == "ifdef":
        return _net_ifdef(n)
    x = n.relu("tdnn1.relu", n.affine("tdnn1.affine", SPLICE, 32))
    if what == "append_elt":
        x = n.relu("bad.relu", f"Append({x}, Offset({x}, -1))")
    elif what == "ivector_elt":
        n.relu("bad.relu", "ReplaceIndex(ivector, t, 0)")
        x = n.relu("tdnn2.relu", n.affine("tdnn2.affine", f"Append({x}, bad.relu)", 32))
    elif what == "add_log_stddev":
        x = n.norm("bad.renorm", x, add_log_stddev=True)
    elif what == "block_dim":
        x = n.norm("bad.renorm", x, block_dim=8)
    elif what == "terms9":
        x = n.noop("bad.noop", "Sum(" + ", ".join(f"Offset({x}, {o})" if o else x for o in range(-4, 5)) + ")")
    elif what == "stages7":
        for k in range(1, 7):
            x = n.fixed_bias(f"s{k}", x)
    elif what == "const":
        x = n.noop("bad.noop", f"Sum({x}, Const(1, 32))")
    n.output(n.output_affine("output.affine", x))


_NETS = {"refused": _net_refused, "renorm": _net_renorm, "range": _net_range, "chains": _net_chains, "so": _net_so, "sums": _net_sums, "segs": _net_segs,
         "rowwise": _net_rowwise, "ifdef": _net_ifdef}

_FSF3 = {"frame-subsampling-factor": 3}


def _c(net, audio, spec=None, **kw):
    s = dict(dither=0.0)
    s.update(spec or {})
    return dict(spec=s, net=net, graph="grammar", audio=audio, **kw)


CASES = {
    # 1. relu-renorm TDNN: split-fp16 kernels and a row map into the next GEMM's image (128), a ragged last 64-column step (100, 65),
    # fewer columns than lanes (33), a layer of all-zero rows (kSquaredNormFloor decides)
    "ff_renorm128": _c(("renorm", dict(width=128)), "synth:110:24000"),
    "ff_renorm100": _c(("renorm", dict(width=100)), "synth:111:24000"),
    "ff_renorm65": _c(("renorm", dict(width=65)), "synth:112:24000"),
    "ff_renorm33": _c(("renorm", dict(width=33)), "synth:113:24000"),
    "ff_renorm_floor": _c(("renorm", dict(width=65, floor=True)), "synth:114:24000"),
    # 2. row-wise on a column range; log-softmax at 65 and 130 pdfs
    "ff_range65": _c(("range", {}), "synth:115:24000", spec=dict(num_phones=65, chain_topology=False)),
    "ff_range130": _c(("range", {}), "synth:116:24000", spec=dict(num_phones=65)),
    # 3. stage chains behind the layer GEMMs (split-fp16 at 128, the exact kernels at 64) and as an op of their own
    "ff_chains128_r0": _c(("chains", dict(width=128, rot=0)), "synth:117:24000"),
    "ff_chains128_r1": _c(("chains", dict(width=128, rot=1)), "synth:118:24000"),
    "ff_chains128_r2": _c(("chains", dict(width=128, rot=2)), "synth:119:24000"),
    "ff_chains128_r3": _c(("chains", dict(width=128, rot=3)), "synth:120:24000"),
    "ff_chains64_r0": _c(("chains", dict(width=64, rot=0)), "synth:121:24000"),
    "ff_chains64_r2": _c(("chains", dict(width=64, rot=2)), "synth:122:24000"),
    # 4. the scale / offset components, each fused and on its own
    "ff_so": _c(("so", {}), "synth:123:24000"),
    # 5. sums
    "ff_sums": _c(("sums", {}), "synth:124:24000"),
    # 6. 16 segments and the aliased output
    "ff_segs16": _c(("segs", {}), "synth:125:24000"),
    # 7. row-wise components in the positions that used to end every decode call in RunNnet's error
    "ff_rw_relu": _c(("rowwise", dict(form="relu")), "synth:126:24000"),
    "ff_rw_bn": _c(("rowwise", dict(form="bn")), "synth:127:24000"),
    "ff_rw_sum": _c(("rowwise", dict(form="sum")), "synth:128:24000"),
    "ff_rw_lsm_scale": _c(("rowwise", dict(form="lsm_scale")), "synth:129:24000"),
    "ff_rw_sum_off": _c(("rowwise", dict(form="sum_off")), "synth:130:24000"),
    # 8. IfDefined outside a cycle: decoded by the reference, refused by the library (REFUSED["ifdef"])
    "ff_ifdef": _c(("ifdef", {}), "synth:131:24000"),
    # 9. --frame-subsampling-factor=3 (strided and trimmed row lists) and the length edges
    "ff_renorm128_fsf3": _c(("renorm", dict(width=128)), "synth:132:24000", conf_opts=_FSF3),
    "ff_range130_fsf3": _c(("range", {}), "synth:133:24000", spec=dict(num_phones=65), conf_opts=_FSF3),
    "ff_sums_fsf3": _c(("sums", {}), "synth:134:24000", conf_opts=_FSF3),
    "ff_rw_relu_fsf3": _c(("rowwise", dict(form="relu")), "synth:135:24000", conf_opts=_FSF3),
    "ff_rw_sum_off_fsf3": _c(("rowwise", dict(form="sum_off")), "synth:140:24000", conf_opts=_FSF3),
    "ff_rw_lsm_scale_fsf3": _c(("rowwise", dict(form="lsm_scale")), "synth:137:24000", conf_opts=_FSF3),
    "ff_range65_fsf3": _c(("range", {}), "synth:141:24000", spec=dict(num_phones=65, chain_topology=False), conf_opts=_FSF3),
    "ff_rw_bn_fsf3": _c(("rowwise", dict(form="bn")), "synth:142:24000", conf_opts=_FSF3),
    "ff_rw_sum_fsf3": _c(("rowwise", dict(form="sum")), "synth:144:24000", conf_opts=_FSF3),
    "ff_renorm128_len0": _c(("renorm", dict(width=128)), "synth:138:399"),
    "ff_renorm128_len1": _c(("renorm", dict(width=128)), "synth:139:400"),
}
ROWWISE = ("ff_rw_relu", "ff_rw_bn", "ff_rw_sum", "ff_rw_lsm_scale", "ff_rw_sum_off")
NO_FRAME = ("ff_renorm128_len0",)
NO_LOAD = ("ff_ifdef",)
# the dense case of the same model for a factor-3 case
DENSE_OF = {n: n[:-5] for n in CASES if n.endswith("_fsf3")}


def model_key(name: str):
    """Cases with the same key decode with one model and one graph."""
    c = CASES[name]
    return repr((sorted(c["spec"].items(), key=str), c["net"], c["graph"], c.get("conf_opts"), c.get("opts")))


def net_key(name: str):
    c = CASES[name]
    return repr((sorted(c["spec"].items(), key=str), c["net"]))


def fsf_of(name: str) -> int:
    return int(CASES[name].get("conf_opts", {}).get("frame-subsampling-factor", 1))


def build_net(name_or_net, spec=None) -> Net:
    """The case's network (or that of a (builder, kwargs) pair on `spec`): seeded by the spec, so the same wherever it is built."""
    if isinstance(name_or_net, str):
        spec = cases.case_spec(CASES[name_or_net])
        name_or_net = CASES[name_or_net]["net"]
    n = Net(spec, spec.seed)
    _NETS[name_or_net[0]](n, **name_or_net[1])
    return n


def write_case_model(case: dict, root: Path):
    """(model_dir, graph_dir, wav, pcm) of a case dictionary under `root`: tests/cases.py's files with the case's own network in final.mdl."""
    model_dir, graph_dir, wav, pcm = cases.build_case_files(case, root)
    spec = cases.case_spec(case)
    n = build_net(case["net"], spec)
    synth.write_final_mdl(model_dir / "model" / "model" / "final.mdl", spec, nnet=(n.cfg, n.comps))
    return model_dir, graph_dir, wav, pcm


def build_case_files(name: str, root: Path):
    """(model_dir, graph_dir, wav, pcm) of the case under `root`."""
    return write_case_model(CASES[name], root)


def load_golden(name: str):
    return np.load(GOLDEN / f"{name}.npz")


# ------------------------------------------------------------------------------------------ float64 restatement

def ensure_nonzero(s):
    """cu::EnsureNonzero (cu-math.cc:226-238) on a float32 vector, in float64."""
    s = np.asarray(s, np.float64)
    return np.where((s <= -_EPSILON) | (s >= _EPSILON), s, np.where(s >= 0.0, _EPSILON, -_EPSILON))


def parse_nodes(cfg):
    nodes = {}
    for ln in cfg:
        first, rest = ln.split(None, 1)
        keys = [(m.start(1), m.end()) for m in re.finditer(r"(?:^|\s)([\w-]+)=", rest)]
        kv = {rest[ks:ve - 1]: rest[ve:(keys[i + 1][0] if i + 1 < len(keys) else len(rest))].strip() for i, (ks, ve) in enumerate(keys)}
        kv["_type"] = first
        nodes[kv["name"]] = kv
    return nodes


class Float64Net:
    """A network of this module in float64, straight from its definition.  A value is (first t at which the node is computable, its
    rows from that t on); the input is replicated at both edges as the reference's decodable pads it, further than any case's context.
    The switches break one feature each: the tests use them to show that a case's log-likelihoods tell the difference."""

    HALO = 24
    swap = None                   # (node a, node b): each is evaluated with the other's component (stages in the other order)
    no_offset = None              # (node, k): the k-th Offset() of that node's descriptor is dropped
    no_scale = None               # (node, k): the k-th Scale() of that node's descriptor is dropped
    norm_floor = True             # kSquaredNormFloor applied
    col0_zero = False             # dim-range-nodes read from column 0
    use_target_rms = True
    apply_ensure_nonzero = True

    def __init__(self, net: Net):
        self.comps = {}
        for name, fn in net.comps:
            r = _Recorder()
            fn(r)
            self.comps[name] = (next(iter(r.fields))[1:-1], r.fields)
        self.nodes = parse_nodes(net.cfg)

    @staticmethod
    def _align(vals):
        t0 = max(v[0] for v in vals)
        rows = [v[1][t0 - v[0]:] for v in vals]
        n = min(r.shape[0] for r in rows)
        return t0, [r[:n] for r in rows]

    def _desc(self, s, ctx):
        """ctx: [node, Offset()s seen, Scale()s seen] of the descriptor being evaluated."""
        fn, args = _call(s)
        if fn in ("Append", "Sum"):
            t0, rows = self._align([self._desc(a, ctx) for a in args])
            return (t0, np.concatenate(rows, axis=1)) if fn == "Append" else (t0, sum(rows))
        if fn == "Offset":
            k = ctx[1]
            ctx[1] += 1
            t0, a = self._desc(args[0], ctx)
            o = 0 if self.no_offset == (ctx[0], k) else int(args[1])
            return t0 - o, a      # x[t + o]: row i of the result is t = t0 - o + i
        if fn == "Scale":
            k = ctx[2]
            ctx[2] += 1
            t0, a = self._desc(args[1], ctx)
            return t0, (1.0 if self.no_scale == (ctx[0], k) else float(np.float32(float(args[0])))) * a
        if fn is not None:      # ReplaceIndex(ivector, t, 0): the iVector rows are constant over t already
            return self._desc(args[0], ctx)
        return self._node(s.strip())

    def _apply(self, typ, f, x):
        if typ in ("NaturalGradientAffineComponent", "AffineComponent", "FixedAffineComponent"):
            return x @ f["<LinearParams>"][0].T + f["<BiasParams>"][0][None, :]
        if typ == "RectifiedLinearComponent":
            return np.maximum(x, 0.0)
        if typ == "NoOpComponent":
            return x
        if typ == "BatchNormComponent":
            mean, var = f["<StatsMean>"][0], f["<StatsVar>"][0]
            scale = f["<TargetRms>"][0] / np.sqrt(var + f["<Epsilon>"][0])
            return x * scale[None, :] + (-mean * scale)[None, :]
        if typ == "BackpropTruncationComponent":
            return float(np.float32(f["<Scale>"][0])) * x
        if typ == "NormalizeComponent":
            # nnet-normalize-component.cc:113-129 -> cu::NormalizePerRow: x * max(sum(x^2) / (D rms^2), floor)^-0.5
            rms = float(np.float32(f["<TargetRms>"][0])) if self.use_target_rms else 1.0
            ss = (x * x).sum(1) / (x.shape[1] * rms * rms)
            with np.errstate(divide="ignore", invalid="ignore"):
                return x * np.power(np.maximum(ss, _NORM_FLOOR) if self.norm_floor else ss, -0.5)[:, None]
        if typ == "LogSoftmaxComponent":
            mx = x.max(1, keepdims=True)
            return x - mx - np.log(np.exp(x - mx).sum(1, keepdims=True))
        if typ == "FixedScaleComponent":
            return x * f["<Scales>"][0][None, :]
        if typ in ("PerElementScaleComponent", "NaturalGradientPerElementScaleComponent"):
            return x * f["<Params>"][0][None, :]
        if typ == "FixedBiasComponent":
            return x + f["<Bias>"][0][None, :]
        if typ == "PerElementOffsetComponent":
            return x + np.tile(f["<Offsets>"][0], x.shape[1] // f["<Offsets>"][0].shape[0])[None, :]
        if typ == "ScaleAndOffsetComponent":
            s = f["<Scales>"][0]
            s = ensure_nonzero(s) if self.apply_ensure_nonzero else s
            rep = x.shape[1] // s.shape[0]      # (the block form: the vectors repeat along the row)
            return x * np.tile(s, rep)[None, :] + np.tile(f["<Offsets>"][0], rep)[None, :]
        raise ValueError(typ)

    def _node(self, name):
        if name in self.memo:
            return self.memo[name]
        kv = self.nodes[name]
        if kv["_type"] == "dim-range-node":
            t0, a = self._node(kv["input-node"])
            o, d = 0 if self.col0_zero else int(kv["dim-offset"]), int(kv["dim"])
            out = (t0, a[:, o:o + d])
        elif kv["_type"] == "output-node":
            out = self._desc(kv["input"], [name, 0, 0])
        else:
            comp = kv["component"]
            if self.swap and name in self.swap:
                comp = self.nodes[self.swap[1 - self.swap.index(name)]]["component"]
            typ, f = self.comps[comp]
            t0, x = self._desc(kv["input"], [name, 0, 0])
            if typ == "TdnnComponent":
                # out[t] = b + sum_i W_i x[t + o_i] (nnet-tdnn-component.cc:208-242): the input's rows at each offset, side by side
                t0, rows = self._align([(t0 - int(o), x) for o in f["<TimeOffsets>"][0]])
                out = (t0, np.concatenate(rows, axis=1) @ f["<LinearParams>"][0].T + f["<BiasParams>"][0][None, :])
            else:
                out = (t0, self._apply(typ, f, x))
        self.memo[name] = out
        return out

    def forward(self, feats, ivector):
        """feats: T x C `input` rows; ivector: the one row every frame sees.  Returns T x pdfs log-likelihoods."""
        T, H = feats.shape[0], self.HALO
        idx = np.clip(np.arange(-H, T + H), 0, T - 1)
        self.memo = {"input": (-H, np.asarray(feats, np.float64)[idx]),
                     "ivector": (-H, np.tile(np.asarray(ivector, np.float64).reshape(1, -1), (T + 2 * H, 1)))}
        t0, out = self._node("output")
        assert t0 <= 0 and out.shape[0] + t0 >= T, (t0, out.shape)
        return out[-t0:-t0 + T]


def restate(name: str, g=None, feats=None, ivector=None, **switches):
    """Log-likelihoods of the case as the reference lays them out, in float64, from its golden's input rows and iVector (or from the
    rows given).  switches: Float64Net's."""
    g = load_golden(name) if g is None and feats is None else g
    net = Float64Net(build_net(name))
    for k, v in switches.items():
        assert hasattr(Float64Net, k), k
        setattr(net, k, v)
    feats = g["input"] if feats is None else feats
    ivector = g["offline_ivector"][0] if ivector is None else ivector
    return net.forward(feats, ivector)[::fsf_of(name)]


# ------------------------------------------------------------------------------------------ the lowering, restated

_AFFINE = ("AffineComponent", "NaturalGradientAffineComponent", "FixedAffineComponent", "LinearComponent", "TdnnComponent")
_ROWWISE = ("LogSoftmaxComponent", "NormalizeComponent")


def _stages_of(typ, f):
    """The elementwise stages of a component: a list of "row" (a row-wise stage) / "elt", or None for a type that is none."""
    if typ in ("NoOpComponent", "DropoutComponent", "GeneralDropoutComponent"):
        return []
    if typ == "BackpropTruncationComponent":
        return [] if float(np.float32(f["<Scale>"][0])) == 1.0 else ["elt"]
    if typ in _ROWWISE:
        return ["row"]
    if typ in ("RectifiedLinearComponent", "BatchNormComponent", "FixedScaleComponent", "PerElementScaleComponent", "FixedBiasComponent",
               "NaturalGradientPerElementScaleComponent", "PerElementOffsetComponent", "ScaleAndOffsetComponent"):
        return ["elt"]
    return None


def _terms(desc):
    """The parts of a node's descriptor, each a list of terms (node, offset, scale): Append at the top, a Sum per part, Offset and
    Scale in any nesting inside."""
    def term(s, off, scale):
        fn, args = _call(s)
        if fn == "Offset":
            return term(args[0], off + int(args[1]), scale)
        if fn == "Scale":
            return term(args[1], off, scale * float(np.float32(float(args[0]))))
        if fn in ("ReplaceIndex", "IfDefined"):
            return term(args[0], off, scale)
        assert fn is None, s
        return [(s.strip(), off, scale)]

    def part(s, off=0, scale=1.0):
        fn, args = _call(s)
        if fn == "Sum":
            return [t for a in args for t in part(a, off, scale)]
        if fn == "Offset":
            return part(args[0], off + int(args[1]), scale)
        if fn == "Scale":
            return part(args[1], off, scale * float(np.float32(float(args[0]))))
        return term(s, off, scale)
    fn, args = _call(desc)
    return [part(a) for a in args] if fn == "Append" else [part(desc)]


def net_ops(net: Net, fsf: int = 1, fuse_residual: bool = True):
    """The ops Nnet::Compile makes of the network, in order, as dictionaries: kind ("gemm" / "eltwise"), name (with its +fused parts),
    out_dim, stages (a count), for a gemm segs [(row offset, columns)] and res (a folded residual's scale or None), for an eltwise op
    terms (a count); stride (fsf where nothing reads the rows between, as `rows=every-<fsf>` says).  Restated from the rules, not the
    code: a node is visited after what it reads, depth first from the output in descriptor order; an elementwise node joins the op
    that made its only source when it reads all of it plainly, unless it is row-wise or brings a stage to a row-wise op; a part of an affine's Append that is
    a Sum() or carries a Scale() becomes <node>.sum first, once; so does the input of a row-wise node; an output-node that names a
    whole buffer without an op to join is an alias; a stage-less two-term op whose unscaled term is a layer GEMM's otherwise unread
    result, the other term made earlier, becomes that GEMM's residual."""
    nodes = parse_nodes(net.cfg)
    ctype = {}
    for name, fn in net.comps:
        r = _Recorder()
        fn(r)
        ctype[name] = (next(iter(r.fields))[1:-1], r.fields)
    order, seen = [], set()

    def visit(n):
        if n in seen:
            return
        seen.add(n)
        kv = nodes[n]
        if kv["_type"] == "dim-range-node":
            visit(kv["input-node"])
        elif kv["_type"] != "input-node":
            for p in _terms(kv["input"]):
                for t in p:
                    visit(t[0])
        order.append(n)
    visit("output")
    consumers = {n: 0 for n in nodes}
    for n in order:
        kv = nodes[n]
        if kv["_type"] == "dim-range-node":
            consumers[kv["input-node"]] += 2
        elif kv["_type"] != "input-node":
            for p in _terms(kv["input"]):
                for t in p:
                    consumers[t[0]] += 1
    ops, bufs = [], [net.dims["input"]]            # bufs: the buffers' widths
    node_buf, node_col, node_op = {"input": 0, "ivector": -2}, {"input": 0, "ivector": 0}, {}

    def new_buf(dim):
        bufs.append(dim)
        return len(bufs) - 1

    def sum_op(n, part, dim):
        op = dict(kind="eltwise", name=n + ".sum", out_dim=dim, stages=0, rows=[], terms=[(node_buf[t], node_col[t], off, sc) for t, off, sc in part],
                  out=new_buf(dim), res=None)
        ops.append(op)
        return op["out"]

    for n in order:
        kv = nodes[n]
        if kv["_type"] == "input-node":
            continue
        if kv["_type"] == "dim-range-node":
            node_buf[n], node_col[n] = node_buf[kv["input-node"]], node_col[kv["input-node"]] + int(kv["dim-offset"])
            continue
        typ, f = ctype[kv["component"]] if kv["_type"] == "component-node" else (None, None)
        parts = _terms(kv["input"])
        stages = [] if typ is None else _stages_of(typ, f)
        if typ in _AFFINE:
            toffs = [int(o) for o in f["<TimeOffsets>"][0]] if typ == "TdnnComponent" else [0]
            op = dict(kind="gemm", name=n, out_dim=net.dims[n], stages=0, rows=[], segs=[], res=None)
            made = {}
            for o2 in toffs:
                for pi, p in enumerate(parts):
                    dim = net.dims[p[0][0]]
                    if len(p) == 1 and p[0][2] == 1.0:
                        t, off, _ = p[0]
                        op["segs"].append((-1, 0, 0, dim) if node_buf[t] == -2 else (node_buf[t], node_col[t], off + o2, dim))
                    else:
                        if pi not in made:
                            made[pi] = sum_op(n, p, dim)
                        op["segs"].append((made[pi], 0, o2, dim))
            op["out"] = new_buf(net.dims[n])
            ops.append(op)
            node_buf[n], node_col[n], node_op[n] = op["out"], 0, op
            continue
        assert stages is not None, typ
        assert len(parts) == 1, "Append() feeding a non-affine component"
        p = parts[0]
        if len(p) == 1:
            t, off, sc = p[0]
            src = node_op.get(t)
            if (off == 0 and sc == 1.0 and consumers[t] == 1 and src is not None and node_col[t] == 0 and nodes[t]["_type"] != "dim-range-node"
                    and "row" not in stages and not (src.get("row") and stages)):
                src["stages"] += len(stages)
                src["name"] += "+" + n
                node_buf[n], node_col[n], node_op[n] = node_buf[t], 0, src
                continue
        dim = net.dims[p[0][0]]
        terms = [(node_buf[t], node_col[t], off, sc) for t, off, sc in p]
        if "row" in stages and (len(terms) != 1 or terms[0][3] != 1.0):
            terms = [(sum_op(n, p, dim), 0, 0, 1.0)]
        if (kv["_type"] == "output-node" and len(terms) == 1 and terms[0][1:] == (0, 0, 1.0) and bufs[terms[0][0]] == dim and not stages):
            node_buf[n], node_col[n] = terms[0][0], 0
            continue
        op = dict(kind="eltwise", name=n, out_dim=dim, stages=len(stages), rows=[], terms=terms, out=new_buf(dim), res=None, row="row" in stages)
        ops.append(op)
        node_buf[n], node_col[n], node_op[n] = op["out"], 0, op
    out_buf = node_buf["output"]

    def reads(op):
        r = [(b, off) for b, _c, off, *_ in op.get("segs", []) if b >= 0] + [(b, off) for b, _c, off, _s in op.get("terms", [])]
        return r + ([(op["res_buf"], 0)] if op["res"] is not None else [])

    # the residual fold
    ei = 0
    while fuse_residual and ei < len(ops):
        eo = ops[ei]
        ei += 1
        if eo["kind"] != "eltwise" or len(eo["terms"]) != 2 or eo["stages"]:
            continue
        for k in (0, 1):
            t, r = eo["terms"][k], eo["terms"][1 - k]
            if t[3] != 1.0 or t[2] != 0 or r[2] != 0 or t[1] != 0 or r[1] != 0 or t[0] == r[0]:
                continue
            if bufs[t[0]] != eo["out_dim"] or bufs[r[0]] != eo["out_dim"]:
                continue
            if sum(b == t[0] for o in ops for b, _ in reads(o)) + (t[0] == out_buf) != 1:
                continue
            gi = next((i for i in range(ei - 1) if ops[i]["out"] == t[0]), None)
            ri = next((i for i in range(ei - 1) if ops[i]["out"] == r[0]), None)
            if gi is None or ops[gi]["kind"] != "gemm" or ops[gi]["res"] is not None or (r[0] != 0 and (ri is None or ri >= gi)):
                continue
            g = ops[gi]
            g["res"], g["res_buf"], g["out"] = r[3], r[0], eo["out"]
            g["name"] += "+" + eo["name"]
            ei -= 1
            del ops[ei]
            break
    # the rows each buffer is read at, modulo the subsampling factor
    need = {b: set() for b in range(len(bufs))}
    need[out_buf].add(0)
    for op in reversed(ops):
        for b, off in reads(op):
            need[b] |= {(r + off) % fsf for r in need[op["out"]]}
    for op in ops:
        op["stride"] = fsf if fsf > 1 and need[op["out"]] == {0} else 1
    return ops


def op_line(op) -> str:
    """The op as rs_model_describe prints it, without the buffer numbers of a gemm's segments."""
    s = f"op: {op['kind']} {op['name']} out_dim={op['out_dim']}"
    if op["kind"] == "gemm":
        s += " segs=" + "".join(f"[{off}:{n}]" for _b, _c, off, n in op["segs"]) + (f" residual={op['res']:g}" if op["res"] is not None else "")
    else:
        s += f" terms={len(op['terms'])}"
    return s + f" stages={op['stages']}" + (f" rows=every-{op['stride']}" if op["stride"] > 1 else "")


def described_ops(text: str):
    """The `op:` lines of a model's description in op_line's form."""
    out = []
    for l in text.splitlines():
        if l.startswith("op: "):
            l = re.sub(r" k=\d+", "", l)
            l = re.sub(r"\[-?\d+:(-?\d+):(\d+)\]", r"[\1:\2]", l)
            out.append(re.sub(r" residual=([^*]+)\*\[\d+\]", r" residual=\1", l))
    return out
