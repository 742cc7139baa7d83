"""Synthetic "zamia-like" model / graph / audio generator in genuine Kaldi on-disk formats.

No acoustic model, HCLG or config ships with the reference, so the
benchmark and the parity tests run on synthetic models written in exactly the layout
the reference's hot path reads:

    <model_dir>/model/model/final.mdl                         TransitionModel + nnet3 (binary or text)
    <model_dir>/model/online/conf/{online,mfcc,ivector_extractor,splice,online_cmvn}.conf      (fbank.conf for mfcc.conf: ModelSpec.feature_type)
    <model_dir>/model/online/ivector_extractor/{final.mat,final.ie,final.dubm,global_cmvn.stats}
    <graph_dir>/{HCLG.fst,words.txt}

Formats follow kaldi/src/base/io-funcs-inl.h (binary basic types), matrix/kaldi-matrix.cc
(FM/FV/DM/DV/DP), hmm/transition-model.cc:422-453, hmm/hmm-topology.cc:163-230,
nnet3/nnet-nnet.cc:631-656, nnet3/am-nnet-simple.cc:33-45, gmm/diag-gmm.cc (Write),
ivector/ivector-extractor.cc:805-825, openfst const-fst.h (ConstFst v2).  The files are
validated by the reference's own binaries in tests (oracle/_ref) in the build container.

Everything here is plain numpy; it runs on the GPU box (no Kaldi needed).
"""
from __future__ import annotations

import io
import math
import struct
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# --------------------------------------------------------------------------- binary/text writers


class KaldiWriter:
    """Minimal Kaldi object writer (binary or text)."""

    def __init__(self, binary: bool = True):
        self.binary = binary
        self.buf = io.BytesIO()
        if binary:
            self.buf.write(b"\0B")

    def token(self, tok: str) -> "KaldiWriter":
        self.buf.write(tok.encode() + b" ")
        return self

    def nl(self) -> "KaldiWriter":
        if not self.binary:
            self.buf.write(b"\n")
        return self

    def raw(self, b: bytes) -> "KaldiWriter":
        self.buf.write(b)
        return self

    def i32(self, v: int) -> "KaldiWriter":
        if self.binary:
            self.buf.write(b"\x04" + struct.pack("<i", int(v)))
        else:
            self.buf.write(f"{int(v)} ".encode())
        return self

    def f32(self, v: float) -> "KaldiWriter":
        if self.binary:
            self.buf.write(b"\x04" + struct.pack("<f", float(v)))
        else:
            self.buf.write(f"{float(np.float32(v))!r} ".encode())
        return self

    def f64(self, v: float) -> "KaldiWriter":
        if self.binary:
            self.buf.write(b"\x08" + struct.pack("<d", float(v)))
        else:
            self.buf.write(f"{float(v)!r} ".encode())
        return self

    def boolean(self, v: bool) -> "KaldiWriter":
        self.buf.write(b"T" if v else b"F")
        if not self.binary:
            self.buf.write(b" ")
        return self

    def int_vector(self, v: Sequence[int]) -> "KaldiWriter":
        if self.binary:
            self.buf.write(b"\x04" + struct.pack("<i", len(v)))
            self.buf.write(np.asarray(v, dtype="<i4").tobytes())
        else:
            self.buf.write(("[ " + " ".join(str(int(x)) for x in v) + " ]\n").encode())
        return self

    def int_pair_vector(self, v: Sequence[Tuple[int, int]]) -> "KaldiWriter":
        """WriteIntegerPairVector (base/io-funcs-inl.h:93-127)."""
        if self.binary:
            self.buf.write(b"\x04" + struct.pack("<i", len(v)))
            self.buf.write(np.asarray(v, dtype="<i4").reshape(-1).tobytes())
        else:
            self.buf.write(("[ " + "".join(f"{int(a)},{int(b)} " for a, b in v) + "]\n").encode())
        return self

    def vector(self, v: np.ndarray, double: bool = False) -> "KaldiWriter":
        v = np.asarray(v)
        if self.binary:
            self.buf.write((b"DV " if double else b"FV ") + b"\x04" + struct.pack("<i", v.shape[0]))
            self.buf.write(v.astype("<f8" if double else "<f4").tobytes())
        else:
            vals = v.astype(np.float64 if double else np.float32)
            self.buf.write((" [ " + " ".join(repr(float(x)) for x in vals) + " ]\n").encode())
        return self

    def matrix(self, m: np.ndarray, double: bool = False) -> "KaldiWriter":
        m = np.asarray(m)
        if self.binary:
            self.buf.write((b"DM " if double else b"FM ") + b"\x04" + struct.pack("<i", m.shape[0])
                           + b"\x04" + struct.pack("<i", m.shape[1]))
            self.buf.write(np.ascontiguousarray(m.astype("<f8" if double else "<f4")).tobytes())
        else:
            vals = m.astype(np.float64 if double else np.float32)
            if vals.shape[0] == 0:
                self.buf.write(b" [ ]\n")
            else:
                rows = ["  " + " ".join(repr(float(x)) for x in r) for r in vals]
                self.buf.write((" [\n" + "\n".join(rows) + " ]\n").encode())
        return self

    def sp_matrix(self, m: np.ndarray, double: bool = True) -> "KaldiWriter":
        """Packed symmetric matrix (lower triangle, row-major): DP/FP."""
        n = m.shape[0]
        packed = m[np.tril_indices(n)]
        if self.binary:
            self.buf.write((b"DP " if double else b"FP ") + b"\x04" + struct.pack("<i", n))
            self.buf.write(packed.astype("<f8" if double else "<f4").tobytes())
        else:
            out = [" ["]
            k = 0
            for r in range(n):
                out.append("  " + " ".join(repr(float(x)) for x in packed[k:k + r + 1]))
                k += r + 1
            self.buf.write(("\n".join(out) + " ]\n").encode())
        return self

    def getvalue(self) -> bytes:
        return self.buf.getvalue()


def write_kaldi_matrix_file(path: Path, m: np.ndarray, binary: bool = True, double: bool = False) -> None:
    w = KaldiWriter(binary)
    w.matrix(m, double)
    Path(path).write_bytes(w.getvalue())


# --------------------------------------------------------------------------- model spec


@dataclass
class ModelSpec:
    """Dimensions of a synthetic acoustic model.  Defaults = "zamia-like-S" (SURVEY.md §8(d))."""

    name: str = "zamia-like-S"
    seed: int = 1
    num_ceps: int = 40
    num_mel_bins: int = 40
    ivector_dim: int = 100          # 0 => no iVector extractor at all
    num_gauss: int = 512
    lda_dim: int = 40
    splice_left: int = 3
    splice_right: int = 3
    num_phones: int = 1000          # chain topology: 2 pdfs per phone => P = 2*num_phones
    hidden_dim: int = 250
    # per hidden layer: time offsets of its input Append
    layer_offsets: Tuple[Tuple[int, ...], ...] = ((0,), (-1, 0, 1), (-1, 0, 1), (-3, 0, 3), (-3, 0, 3), (-3, 0, 3), (-3, 0, 3))
    lda_offsets: Tuple[int, ...] = (-1, 0, 1)
    prefinal_dim: int = 250
    with_priors: bool = False
    with_log_softmax: bool = False
    tdnnf: bool = False              # use TdnnComponent + LinearComponent bottlenecks (coverage net)
    bottleneck_dim: int = 64
    chain_topology: bool = True      # forward/self-loop pdf classes (nnet3 chain models)
    dither: Optional[float] = None   # None: no --dither line, i.e. the reference's default 1.0 like conf/mfcc_hires.conf (feature-window.h:57)
    frame_length: Optional[float] = None   # ms; None: no --frame-length line (25 ms: a 512-point FFT); 100 ms pads to 2048 points
    # --sample-frequency of mfcc.conf / fbank.conf (8000: a 200-sample window, the 256-point FFT; 22050 / 32000: 1024 points) and the
    # band of the mel banks, None: --low-freq=20 / --high-freq=-400 as for 16 kHz (Kaldi's mfcc_hires for 8 kHz has 40 and -200)
    sample_frequency: int = 16000
    low_freq: Optional[float] = None
    high_freq: Optional[float] = None
    # mfcc.conf holds --sample-frequency and --use-energy=false and nothing else: the reference's defaults for the rest (23 bins,
    # 13 cepstra, which num_mel_bins / num_ceps then have to say; low-freq 20, high-freq 0, dither 1.0)
    mfcc_defaults: bool = False
    nnet_cmvn: bool = False          # --cmvn-config on the nnet input branch
    binary: bool = True
    xent_branch: bool = True         # extra output-xent branch (ignored by decoding), as chain recipes have
    input_scale: float = 0.04        # lda columns that see raw MFCCs (magnitude ~10-80) are scaled down, like a trained LDA whitens
    output_scale: float = 0.25       # keeps per-frame log-likelihood spread at a realistic few units
    # phonetic context of the decision tree written beside final.mdl (graph construction):
    # "mono" (N=1, P=0), "biphone" (N=2, P=1: every third phone has two pdf sets chosen by its left neighbour) or
    # "triphone" (N=3, P=1: additionally every third phone is split on its right neighbour)
    context: str = "mono"
    # layer weights: "normal" = N(0, 1 / fan_in); "heavy" = Student t with 2 degrees of freedom / sqrt(fan_in), clipped to
    # +-1000: rows with a few weights hundreds of times the typical one (the split-precision GEMMs scale every output column by
    # its largest weight)
    weight_dist: str = "normal"
    hidden_gain: float = 1.0         # the second hidden layer's weights times this (activations beyond fp16's range for ~1e5)
    # hidden_gain with the rest of the network making up for it: the second hidden layer's bias is scaled too, it has no BatchNorm
    # (its output is relu(gain * (W x + b)): every element of every row is of order gain), and the third layer's weights are
    # divided by gain -- in exact arithmetic the network of gain 1 without that BatchNorm; in a GEMM that carries small operands
    # to a fixed ABSOLUTE error only, a different one (tests: small activations and the split-fp16 layer GEMMs)
    gain_compensated: bool = False
    hmm_states: int = 1              # emitting states per phone (left-to-right; > 1 only with chain_topology = False, graphs by mkgraph)
    # "fbank": log-mel filterbank rows (num_mel_bins bins, + 1 column with use-energy) are the base feature instead of MFCCs;
    # conf/fbank.conf gets the lines the MFCC config would (bins, band, dither, frame length) with fbank_opts' --key=value on top
    # (a key given there replaces the line of that name); fbank_config = False writes no --fbank-config line at all: the
    # reference's defaults (23 bins, dither 1.0), which num_mel_bins then has to match
    feature_type: str = "mfcc"
    fbank_opts: Optional[Dict[str, object]] = None
    fbank_config: bool = True
    # A convolutional front end between the input and the first affine (nnet3's CNN-TDNN recipes: conv-relu-batchnorm-layer).
    # One dict per layer: filters, height_out, sub (height subsampling, default 1) and either time_offsets + height_offsets (the
    # rectangle of both) or offsets (explicit (time, height) pairs); required_time_offsets (default: all of them); gain (default
    # 1: a factor on the layer's weights).  The first layer sees the input as one filter of feat_dim heights, or, with
    # conv_ivector_maps, 1 + conv_ivector_maps filters.  Behind the stack the "lda" FixedAffine maps to hidden_dim.
    conv_layers: Tuple[Dict[str, object], ...] = ()
    conv_idct: bool = False          # idct-layer in front: FixedAffine (feat_dim x feat_dim) + BatchNorm
    # > 0: the iVector goes through a LinearComponent to that many feature maps + BatchNorm, and a PermuteComponent interleaves
    # them with the features (combine-feature-maps-layer) instead of being appended to the first affine's input
    conv_ivector_maps: int = 0
    # Recurrent blocks between the TDNN layers (nnet3's fast-lstmp-layer / fast-lstm-layer, xconfig/lstm.py).  One dict per block:
    # after (the block follows that many of layer_offsets' layers, >= 1), cell, rec and nonrec (the recurrent and non-recurrent
    # projection dims; 0 and 0: no projection, fast-lstm-layer), delay (frames towards the past, default 3), scale (the
    # BackpropTruncationComponent's <Scale>, 1 - delay / decay-time in a recipe; default 1), dropout (use-dropout=true with its
    # DropoutMaskComponent node, default False), batchnorm (a BatchNorm on the block's output, default False).
    # form="composed" writes the same cell as separate components, what lstmp-layer / lstmp-batchnorm-layer (batchnorm=True) /
    # lstm-layer (rec = nonrec = 0) emit: dropout is then the shared DropoutComponent behind i, f and o, scale the <Scale> of both
    # truncation components (scale_c / scale_r set them apart), clipgrad=True makes them ClipGradientComponents as older models have.
    # bottleneck=B (with rec = nonrec = 0 and the default form) writes what lstmb-layer emits: the LinearComponents W_all_a (B rows)
    # and W_all_b, the ScaleAndOffsetComponent W_all_b_so, the nonlinearity, cm_trunc and m_batchnorm; self_scale is the Scale() on
    # the recurrent input (default 1); for tests so_scales / so_offsets (tuples, repeated along the 4 cell entries) replace the drawn
    # vectors and wb_gain (default 1) is a factor on W_all_b.
    lstm_layers: Tuple[Dict[str, object], ...] = ()
    # ScaleAndOffsetComponents between the TDNN layers, placed like lstm_layers (behind everything else of the same `after`).  One
    # dict per component: after, block (the length of its vectors; the layer's dim is a multiple of it, default the dim itself).
    scale_offset_layers: Tuple[Dict[str, object], ...] = ()
    # Recurrent blocks of the output-gate projected GRU (nnet3's fast-opgru-layer / fast-norm-opgru-layer, xconfig/gru.py), placed
    # like lstm_layers (behind the LSTM blocks of the same `after`).  One dict per block: after, cell, rec, nonrec (both positive),
    # delay (default 3), scale (the BackpropTruncationComponent's <Scale>, default 1), norm (the norm variant: a NormalizeComponent
    # in the recurrence and a BatchNorm on the output, default False), dropout (norm variant only: the shared DropoutComponent
    # behind the two sigmoids, default False).  form="composed" (default "fast") writes the same cell as separate components, what
    # opgru-layer / norm-opgru-layer emit: Sigmoid / Tanh / ElementwiseProduct nodes, the per-element scale W_h.UW_elementwise and
    # the NoOpComponent y_t, under xconfig's names; the layer's output is then sn_t.
    gru_layers: Tuple[Dict[str, object], ...] = ()
    # Recurrent blocks around a GruNonlinearityComponent (nnet3's fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer,
    # xconfig/gru.py), placed like lstm_layers (behind the OPGRU blocks of the same `after`).  One dict per block: after, cell, rec,
    # nonrec (rec = 0 with nonrec = 0: the plain fast-gru-layer, whose state and output are the cell), delay (default 3), scale
    # (the BackpropTruncationComponent's <Scale>, default 1), norm (fast-norm-pgru-layer: a NormalizeComponent in the recurrence and a
    # BatchNorm on the output, default False), dropout (norm variant only: the two DropoutComponents behind the sigmoids, default
    # False).  form="composed" (default "fast") writes the same cell as separate components, what pgru-layer / norm-pgru-layer /
    # gru-layer (rec = nonrec = 0) emit, under xconfig's names; the layer's output is then sn_t, s_t for gru-layer.
    pgru_layers: Tuple[Dict[str, object], ...] = ()
    # Time-restricted self-attention layers between the TDNN layers (xconfig/attention.py), placed like lstm_layers (behind the
    # recurrent blocks of the same `after`).  One dict per layer: after, heads, key_dim, value_dim, left, right (num-left-inputs,
    # num-right-inputs), stride (time-stride); optional left_required, right_required (default -1: all of them), key_scale (default
    # 1 / sqrt(key_dim)), output_context (default True); form, one of ATTENTION_FORMS (default attention-relu-renorm-layer);
    # logit_gain (default 1: a factor on the key and query rows of the layer's affine, weights and bias).
    attention_layers: Tuple[Dict[str, object], ...] = ()

    @property
    def num_pdfs(self) -> int:
        return len(context_tuples(self)) * (2 if self.chain_topology else 1)

    @property
    def feat_dim(self) -> int:
        """Width of a base-feature row: what the network's input, the extractor's LDA and global_cmvn.stats are sized from."""
        if self.feature_type == "mfcc":
            return self.num_ceps
        if self.feature_type != "fbank":
            raise ValueError(f"feature_type {self.feature_type!r}: mfcc or fbank")
        o = {k: _conf_value(v) for k, v in (self.fbank_opts or {}).items()} if self.fbank_config else {}
        bins = int(o.get("num-mel-bins", self.num_mel_bins)) if self.fbank_config else 23
        return bins + (1 if o.get("use-energy", "false") == "true" else 0)


def _conf_value(v: object) -> str:
    return ("true" if v else "false") if isinstance(v, bool) else str(v)


TINY = dict(name="tiny", ivector_dim=10, num_gauss=16, lda_dim=12, num_phones=24, hidden_dim=32,
            layer_offsets=((0,), (-1, 0, 1), (-2, 0, 2)), prefinal_dim=24)


def tiny_spec(**kw) -> ModelSpec:
    d = dict(TINY)
    d.update(kw)
    return ModelSpec(**d)


# --------------------------------------------------------------------------- phonetic context

def context_shape(spec: "ModelSpec") -> Tuple[int, int]:
    """(context width N, central position P).  Besides the three named shapes any "N,P" is accepted (graph-construction tests)."""
    named = {"mono": (1, 0), "biphone": (2, 1), "triphone": (3, 1)}
    if spec.context in named:
        return named[spec.context]
    n, p = (int(x) for x in spec.context.split(","))
    if not (0 <= p < n):
        raise ValueError(f"bad context {spec.context}")
    return n, p


def context_splits(spec: "ModelSpec", phone: int):
    """None, or (tree key, sorted yes-set) of the one question asked about `phone`'s context window: every third phone is asked
    about its left neighbour (if the window has one), every third about its right neighbour (if it has one)."""
    n = spec.num_phones
    width, central = context_shape(spec)
    if central > 0 and phone % 3 == 0:
        return central - 1, [0] + [q for q in range(1, n + 1) if q % 2 == 1]           # left neighbour (0 = start of utterance)
    if central + 1 < width and phone % 3 == 1:
        return central + 1, [0] + [q for q in range(1, n + 1) if q % 2 == 0]           # right neighbour (0 = end of utterance)
    return None


def variant_pdfs(spec: "ModelSpec") -> Dict[int, List[List[int]]]:
    """phone -> context variants (yes branch first) -> pdf per pdf-class.  Pdf-classes: (forward, self-loop) of the one state of
    the chain topology, or one per emitting state of the HMM topology."""
    if spec.chain_topology and spec.hmm_states != 1:
        raise ValueError("hmm_states > 1 needs chain_topology = False")
    classes = 2 if spec.chain_topology else spec.hmm_states
    out, pdf = {}, 0
    for p in range(1, spec.num_phones + 1):
        out[p] = []
        for _ in range(2 if context_splits(spec, p) else 1):
            out[p].append(list(range(pdf, pdf + classes)))
            pdf += classes
    return out


def context_tuples(spec: "ModelSpec") -> List[Tuple[int, int, int, int]]:
    """The transition model's (phone, hmm-state, forward pdf, self-loop pdf) table, sorted as transition-model.cc:62-100 sorts
    it; a phone with a context question contributes two entries per state."""
    out = []
    for p, variants in variant_pdfs(spec).items():
        for pdfs in variants:
            if spec.chain_topology:
                out.append((p, 0, pdfs[0], pdfs[1]))
            else:
                out += [(p, hs, pdfs[hs], pdfs[hs]) for hs in range(spec.hmm_states)]
    return sorted(out)


def write_tree(path: Path, spec: "ModelSpec") -> None:
    """<model>/tree: a ContextDependency in text form (tree/context-dep.cc:143-156, tree/event-map.cc:55-205): a table on the
    central phone, under it a split on one neighbour where context_splits() asks one, under that the pdf per pdf-class."""
    n_ctx, p_ctx = context_shape(spec)
    vp = variant_pdfs(spec)

    def leaf(pdfs: List[int]) -> str:
        if len(pdfs) == 1:
            return f"CE {pdfs[0]} "
        return f"TE -1 {len(pdfs)} ( " + "".join(f"CE {x} " for x in pdfs) + ") "

    body = f"TE {p_ctx} {spec.num_phones + 1} ( NULL "
    for p in range(1, spec.num_phones + 1):
        q = context_splits(spec, p)
        if q is None:
            body += leaf(vp[p][0])
        else:
            key, yes = q
            body += f"SE {key} [ " + " ".join(map(str, yes)) + " ]\n{ " + leaf(vp[p][0]) + leaf(vp[p][1]) + "} "
    body += ") "
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(f"ContextDependency {n_ctx} {p_ctx} ToPdf {body}\nEndContextDependency ")


# --------------------------------------------------------------------------- final.mdl


def _write_topology(w: KaldiWriter, spec: ModelSpec) -> None:
    phones = list(range(1, spec.num_phones + 1))
    w.token("<Topology>")
    if w.binary:
        w.int_vector(phones)
        phone2idx = [-1] + [0] * spec.num_phones
        w.int_vector(phone2idx)
        if spec.chain_topology:
            w.i32(-1)                    # marker: not a plain HMM (separate self-loop pdf class)
        w.i32(1)                         # one topology entry
        ns = 1 if spec.chain_topology else spec.hmm_states
        w.i32(ns + 1)                    # emitting states + the final one
        for st in range(ns):
            w.i32(st)                    # forward pdf class
            if spec.chain_topology:
                w.i32(1)                 # self-loop pdf class
            w.i32(2)
            w.i32(st).f32(0.5)
            w.i32(st + 1).f32(0.5)
        # final, non-emitting state
        w.i32(-1)
        if spec.chain_topology:
            w.i32(-1)
        w.i32(0)
        w.token("</Topology>")
    else:
        w.raw(b"\n<TopologyEntry>\n<ForPhones>\n" + " ".join(map(str, phones)).encode() + b"\n</ForPhones>\n")
        if spec.chain_topology:
            w.raw(b"<State> 0 <ForwardPdfClass> 0 <SelfLoopPdfClass> 1 <Transition> 0 0.5 <Transition> 1 0.5 </State>\n")
            w.raw(b"<State> 1 </State>\n</TopologyEntry>\n</Topology>\n")
        else:
            for st in range(spec.hmm_states):
                w.raw(f"<State> {st} <PdfClass> {st} <Transition> {st} 0.5 <Transition> {st + 1} 0.5 </State>\n".encode())
            w.raw(f"<State> {spec.hmm_states} </State>\n</TopologyEntry>\n</Topology>\n".encode())


def _write_transition_model(w: KaldiWriter, spec: ModelSpec) -> None:
    w.token("<TransitionModel>").nl()
    _write_topology(w, spec)
    tuples = context_tuples(spec)
    n = len(tuples)
    if spec.chain_topology:
        w.token("<Tuples>").i32(n).nl()
        for p, hs, fwd, slf in tuples:
            w.i32(p).i32(hs).i32(fwd).i32(slf).nl()
        w.token("</Tuples>").nl()
    else:
        w.token("<Triples>").i32(n).nl()
        for p, hs, fwd, _slf in tuples:
            w.i32(p).i32(hs).i32(fwd).nl()
        w.token("</Triples>").nl()
    w.token("<LogProbs>").nl()
    # index 0 unused; one entry per transition-id
    if spec.context == "mono" and spec.hmm_states == 1:
        probs = np.full(2 * n, 0.5)
    else:        # (context-dependent test models: a different self-loop probability per transition-state)
        sl = 0.35 + 0.05 * (np.arange(n) % 7)
        probs = np.stack([sl, 1.0 - sl], axis=1).reshape(-1)
    w.vector(np.concatenate([[0.0], np.log(probs)]).astype(np.float32))
    w.token("</LogProbs>").nl()
    w.token("</TransitionModel>").nl()


def transition_ids(spec: ModelSpec, phone: int) -> Tuple[int, int]:
    """(self-loop tid, forward tid) of 1-based `phone` for the synthetic topology
    (hmm/transition-model.cc:144-177: ids are assigned in tuple order, topology transition order).  Context-independent
    models only: the directly assembled synthetic graphs know nothing of phonetic context."""
    if context_shape(spec) != (1, 0) or spec.hmm_states != 1:
        raise ValueError("transition_ids: context-dependent or multi-state model; build its graph with mkgraph")
    return 2 * (phone - 1) + 1, 2 * (phone - 1) + 2


def tid_to_pdf(spec: ModelSpec) -> np.ndarray:
    tuples = context_tuples(spec)
    out = np.zeros(2 * len(tuples) + 1, dtype=np.int32)
    for k, (_p, _hs, fwd, slf) in enumerate(tuples):
        out[2 * k + 1] = slf         # transition 0 of the topology's state is the self loop
        out[2 * k + 2] = fwd
    return out


def _updatable_open(w: KaldiWriter, typ: str) -> None:
    w.token(f"<{typ}>").token("<LearningRate>").f32(0.001)


def _w_affine(w: KaldiWriter, typ: str, W: np.ndarray, b: np.ndarray) -> None:
    _updatable_open(w, typ)
    w.token("<LinearParams>").matrix(W).token("<BiasParams>").vector(b)
    if typ == "NaturalGradientAffineComponent":
        w.token("<RankIn>").i32(20).token("<RankOut>").i32(80)
        w.token("<UpdatePeriod>").i32(4).token("<NumSamplesHistory>").f32(2000.0).token("<Alpha>").f32(4.0)
    w.token(f"</{typ}>")


def _w_fixed_affine(w: KaldiWriter, W: np.ndarray, b: np.ndarray) -> None:
    w.token("<FixedAffineComponent>").token("<LinearParams>").matrix(W).token("<BiasParams>").vector(b)
    w.token("</FixedAffineComponent>")


def _w_nonlinear(w: KaldiWriter, typ: str, dim: int) -> None:
    w.token(f"<{typ}>").token("<Dim>").i32(dim)
    w.token("<ValueAvg>").vector(np.zeros(0, np.float32)).token("<DerivAvg>").vector(np.zeros(0, np.float32))
    w.token("<Count>").f64(0.0)
    w.token("<OderivRms>").vector(np.zeros(0, np.float32)).token("<OderivCount>").f64(0.0)
    w.token("<NumDimsSelfRepaired>").f64(0.0).token("<NumDimsProcessed>").f64(0.0)
    w.token(f"</{typ}>")


def _w_batchnorm(w: KaldiWriter, mean: np.ndarray, var: np.ndarray, eps: float = 1e-3, target_rms: float = 1.0,
                 dim: Optional[int] = None) -> None:
    """dim: the component's width where it is a multiple of the statistics' (block-dim = their length: one per filter)."""
    block = mean.shape[0]
    dim = block if dim is None else dim
    w.token("<BatchNormComponent>").token("<Dim>").i32(dim).token("<BlockDim>").i32(block)
    w.token("<Epsilon>").f32(eps).token("<TargetRms>").f32(target_rms).token("<TestMode>").boolean(False)
    w.token("<Count>").f32(1000.0).token("<StatsMean>").vector(mean).token("<StatsVar>").vector(var)
    w.token("</BatchNormComponent>")


def _w_tdnn(w: KaldiWriter, offsets: Sequence[int], W: np.ndarray, b: Optional[np.ndarray]) -> None:
    _updatable_open(w, "TdnnComponent")
    w.token("<TimeOffsets>").int_vector(list(offsets))
    w.token("<LinearParams>").matrix(W)
    w.token("<BiasParams>").vector(b if b is not None else np.zeros(0, np.float32))
    w.token("<OrthonormalConstraint>").f32(0.0).token("<UseNaturalGradient>").boolean(True)
    w.token("<NumSamplesHistory>").f32(2000.0).token("<AlphaInOut>").f32(4.0).f32(4.0)
    w.token("<RankInOut>").i32(20).i32(80)
    w.token("</TdnnComponent>")


def conv_layer_offsets(layer: Dict[str, object]) -> List[Tuple[int, int]]:
    """The sorted (time, height) offset pairs of a ModelSpec.conv_layers entry."""
    if "offsets" in layer:
        return sorted((int(t), int(h)) for t, h in layer["offsets"])
    return sorted((int(t), int(h)) for t in layer["time_offsets"] for h in layer["height_offsets"])


def _w_conv(w: KaldiWriter, filters_in: int, filters_out: int, height_in: int, height_out: int, sub: int,
            offsets: Sequence[Tuple[int, int]], required: Sequence[int], W: np.ndarray, b: np.ndarray) -> None:
    # nnet-convolutional-component.cc:424-450 with ConvolutionModel::Write (convolution.cc:225-249)
    _updatable_open(w, "TimeHeightConvolutionComponent")
    w.token("<Model>").token("<ConvolutionModel>")
    w.token("<NumFiltersIn>").i32(filters_in).token("<NumFiltersOut>").i32(filters_out)
    w.token("<HeightIn>").i32(height_in).token("<HeightOut>").i32(height_out).token("<HeightSubsampleOut>").i32(sub)
    w.token("<Offsets>").int_pair_vector(list(offsets))
    w.token("<RequiredTimeOffsets>").int_vector(list(required))
    w.token("</ConvolutionModel>")
    w.token("<LinearParams>").matrix(W).token("<BiasParams>").vector(b)
    w.token("<MaxMemoryMb>").f32(200.0).token("<UseNaturalGradient>").boolean(True)
    w.token("<NumMinibatchesHistory>").f32(4.0).token("<AlphaInOut>").f32(4.0).f32(4.0)
    w.token("<RankInOut>").i32(80).i32(80)
    w.token("</TimeHeightConvolutionComponent>")


def _w_permute(w: KaldiWriter, column_map: Sequence[int]) -> None:
    # nnet-simple-component.cc:4056-4064
    w.token("<PermuteComponent>").token("<ColumnMap>").int_vector(list(column_map)).token("</PermuteComponent>")


def combine_feature_maps(height: int, filters1: int, filters2: int) -> List[int]:
    """combine-feature-maps-layer's column map: the input is Append(a, b), a = height x filters1 and b = height x filters2 (filter
    fastest); output column h * (filters1 + filters2) + f takes a's filter f, or b's filter f - filters1, of height h."""
    out = []
    for h in range(height):
        out += [h * filters1 + f for f in range(filters1)]
        out += [height * filters1 + h * filters2 + f for f in range(filters2)]
    return out


def _w_linear(w: KaldiWriter, W: np.ndarray) -> None:
    _updatable_open(w, "LinearComponent")
    w.token("<Params>").matrix(W)
    w.token("<UseNaturalGradient>").boolean(True).token("<RankInOut>").i32(20).i32(80)
    w.token("<Alpha>").f32(4.0).token("<NumSamplesHistory>").f32(2000.0).token("<UpdatePeriod>").i32(4)
    w.token("</LinearComponent>")


def _w_general_dropout(w: KaldiWriter, dim: int) -> None:
    # nnet-general-component.cc:1674-1696 (test-mode/continuous are bare flag tokens)
    w.token("<GeneralDropoutComponent>").token("<Dim>").i32(dim).token("<BlockDim>").i32(dim)
    w.token("<TimePeriod>").i32(0).token("<DropoutProportion>").f32(0.2)
    w.token("<Continuous>")
    w.token("</GeneralDropoutComponent>")


def _w_noop(w: KaldiWriter, dim: int) -> None:
    # nnet-simple-component.cc:480-487
    w.token("<NoOpComponent>").token("<Dim>").i32(dim).token("<BackpropScale>").f32(1.0).token("</NoOpComponent>")


def _w_lstm_nonlinearity(w: KaldiWriter, params: np.ndarray, use_dropout: bool) -> None:
    # nnet-combined-component.cc:1019-1057 (LstmNonlinearityComponent::Write), behind WriteUpdatableCommon
    cell = params.shape[1]
    _updatable_open(w, "LstmNonlinearityComponent")
    w.token("<Params>").matrix(params)
    w.token("<ValueAvg>").matrix(np.zeros((5, cell), np.float32)).token("<DerivAvg>").matrix(np.zeros((5, cell), np.float32))
    w.token("<SelfRepairConfig>").vector(np.array([0.05, 0.05, 0.2, 0.05, 0.2] + [1e-5] * 5, np.float32))
    w.token("<SelfRepairProb>").vector(np.zeros(5, np.float32))
    if use_dropout:
        w.token("<UseDropout>").boolean(True)
    w.token("<Count>").f64(0.0)
    w.token("</LstmNonlinearityComponent>")


def _w_backprop_truncation(w: KaldiWriter, dim: int, scale: float, recurrence_interval: int) -> None:
    # nnet-general-component.cc:932-955
    w.token("<BackpropTruncationComponent>").token("<Dim>").i32(dim).token("<Scale>").f32(scale)
    w.token("<ClippingThreshold>").f32(30.0).token("<ZeroingThreshold>").f32(15.0).token("<ZeroingInterval>").i32(20)
    w.token("<RecurrenceInterval>").i32(recurrence_interval)
    w.token("<NumElementsClipped>").f64(0.0).token("<NumElementsZeroed>").f64(0.0)
    w.token("<NumElementsProcessed>").f64(0.0).token("<NumZeroingBoundaries>").f64(0.0)
    w.token("</BackpropTruncationComponent>")


def _w_dropout_mask(w: KaldiWriter, output_dim: int, proportion: float = 0.0) -> None:
    # nnet-general-component.cc:1499-1510 (<Continuous> would be a bare flag token)
    w.token("<DropoutMaskComponent>").token("<OutputDim>").i32(output_dim).token("<DropoutProportion>").f32(proportion)
    w.token("<TestMode>").boolean(False)
    w.token("</DropoutMaskComponent>")


def _w_scale_and_offset(w: KaldiWriter, scales: np.ndarray, offsets: np.ndarray, dim: Optional[int] = None) -> None:
    """dim: the component's width where it is a multiple of the vectors' length (its block form)."""
    # nnet-simple-component.cc:2381-2394 (ScaleAndOffsetComponent::Write), behind WriteUpdatableCommon
    _updatable_open(w, "ScaleAndOffsetComponent")
    w.token("<Dim>").i32(scales.shape[0] if dim is None else dim).token("<Scales>").vector(scales).token("<Offsets>").vector(offsets)
    w.token("<UseNaturalGradient>").boolean(True).token("<Rank>").i32(20)
    w.token("</ScaleAndOffsetComponent>")


def lstm_layer_dims(layer: Dict[str, object]) -> Tuple[int, int, int, int]:
    """(cell, recurrent, non-recurrent, output) dims of a ModelSpec.lstm_layers entry; without a projection the recurrent
    input and the output are the cell-wide m."""
    C, R, P = int(layer["cell"]), int(layer.get("rec", 0)), int(layer.get("nonrec", 0))
    if (R == 0) != (P == 0):
        raise ValueError("lstm layer: rec and nonrec are both 0 (no projection) or both positive")
    return C, R, P, (R + P if R else C)


def _lstm_block(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
                prev: str, prev_dim: int) -> Tuple[str, int]:
    """The components and nodes XconfigFastLstmpLayer / XconfigFastLstmLayer emit (xconfig/lstm.py:1120-1198, 706-753), in their
    order.  Returns the node the next layer reads and its dim."""
    if "bottleneck" in layer and (layer.get("form", "fast") != "fast" or int(layer.get("rec", 0)) or int(layer.get("nonrec", 0))):
        raise ValueError("lstm layer: a bottleneck (lstmb-layer) goes with the default form and without a projection")
    if layer.get("form", "fast") == "composed":
        return _lstmp_block(cfg, comps, rng, name, layer, prev, prev_dim)
    if layer.get("form", "fast") != "fast":
        raise ValueError("lstm layer: form is 'fast' (the default) or 'composed'")
    if "bottleneck" in layer:
        return _lstmb_block(cfg, comps, rng, name, layer, prev, prev_dim)
    C, R, P, out_dim = lstm_layer_dims(layer)
    d, scale = int(layer.get("delay", 3)), float(layer.get("scale", 1.0))
    dropout, proj = bool(layer.get("dropout", False)), R > 0
    rec_dim = R if proj else C

    def randn(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    W_all = np.concatenate([randn(4 * C, prev_dim), randn(4 * C, rec_dim)], axis=1)
    b_all = (rng.standard_normal(4 * C) * 0.1).astype(np.float32)
    params = (rng.standard_normal((3, C)) * 0.1).astype(np.float32)
    trunc = "cr_trunc" if proj else "cm_trunc"
    comps.append((f"{name}.W_all", lambda w, W=W_all, b=b_all: _w_affine(w, "NaturalGradientAffineComponent", W, b)))
    comps.append((f"{name}.lstm_nonlin", lambda w, p=params, u=dropout: _w_lstm_nonlinearity(w, p, u)))
    comps.append((f"{name}.{trunc}", lambda w, n=C + rec_dim, s=scale, i=d: _w_backprop_truncation(w, n, s, i)))
    if dropout:
        comps.append((f"{name}.dropout_mask", lambda w: _w_dropout_mask(w, 3)))
    if proj:
        W_rp, b_rp = randn(R + P, C), (rng.standard_normal(R + P) * 0.1).astype(np.float32)
        comps.append((f"{name}.W_rp", lambda w, W=W_rp, b=b_rp: _w_affine(w, "NaturalGradientAffineComponent", W, b)))
    s_r = f"{name}.r_trunc" if proj else f"{name}.m_trunc"
    cfg.append(f"component-node name={name}.W_all component={name}.W_all input=Append({prev}, IfDefined(Offset({s_r}, {-d})))")
    if dropout:
        cfg.append(f"component-node name={name}.dropout_mask component={name}.dropout_mask input={name}.dropout_mask")
        cfg.append(f"component-node name={name}.lstm_nonlin component={name}.lstm_nonlin "
                   f"input=Append({name}.W_all, IfDefined(Offset({name}.c_trunc, {-d})), {name}.dropout_mask)")
    else:
        cfg.append(f"component-node name={name}.lstm_nonlin component={name}.lstm_nonlin "
                   f"input=Append({name}.W_all, IfDefined(Offset({name}.c_trunc, {-d})))")
    if proj:
        cfg.append(f"dim-range-node name={name}.c input-node={name}.lstm_nonlin dim-offset=0 dim={C}")
    cfg.append(f"dim-range-node name={name}.m input-node={name}.lstm_nonlin dim-offset={C} dim={C}")
    if proj:
        cfg.append(f"component-node name={name}.rp component={name}.W_rp input={name}.m")
        cfg.append(f"dim-range-node name={name}.r input-node={name}.rp dim-offset=0 dim={R}")
        cfg.append(f"component-node name={name}.cr_trunc component={name}.cr_trunc input=Append({name}.c, {name}.r)")
        cfg.append(f"dim-range-node name={name}.c_trunc input-node={name}.cr_trunc dim-offset=0 dim={C}")
        cfg.append(f"dim-range-node name={name}.r_trunc input-node={name}.cr_trunc dim-offset={C} dim={R}")
        out = f"{name}.rp"
    else:
        cfg.append(f"component-node name={name}.cm_trunc component={name}.cm_trunc input={name}.lstm_nonlin")
        cfg.append(f"dim-range-node name={name}.c_trunc input-node={name}.cm_trunc dim-offset=0 dim={C}")
        cfg.append(f"dim-range-node name={name}.m_trunc input-node={name}.cm_trunc dim-offset={C} dim={C}")
        out = f"{name}.m"
    if layer.get("batchnorm", False):
        bn = out + "_batchnorm"
        mean, var = (0.1 * rng.standard_normal(out_dim)).astype(np.float32), rng.uniform(0.05, 0.2, out_dim).astype(np.float32)
        comps.append((bn, lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
        cfg.append(f"component-node name={bn} component={bn} input={out}")
        out = bn
    return out, out_dim


def _lstmb_block(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
                 prev: str, prev_dim: int) -> Tuple[str, int]:
    """The components and nodes XconfigLstmbLayer emits (xconfig/lstm.py:901-949), in their order, m_batchnorm included.  Returns
    the node the next layer reads and its dim."""
    C, B = int(layer["cell"]), int(layer["bottleneck"])
    if C <= 0 or B <= 0:
        raise ValueError("lstm layer: cell and bottleneck are positive")
    d, scale, self_scale = int(layer.get("delay", 3)), float(layer.get("scale", 1.0)), float(layer.get("self_scale", 1.0))

    def randn(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def pinned(drawn, key):
        if key not in layer:
            return drawn
        v = np.asarray(layer[key], np.float32)
        return np.resize(v, drawn.shape[0]).astype(np.float32)

    W_a = np.concatenate([randn(B, prev_dim), randn(B, C)], axis=1)
    W_b = randn(4 * C, B) * np.float32(layer.get("wb_gain", 1.0))
    scales = pinned(rng.uniform(0.5, 1.5, 4 * C).astype(np.float32), "so_scales")
    offsets = pinned((rng.standard_normal(4 * C) * 0.1).astype(np.float32), "so_offsets")
    params = (rng.standard_normal((3, C)) * 0.1).astype(np.float32)
    mean, var = (0.1 * rng.standard_normal(C)).astype(np.float32), rng.uniform(0.05, 0.2, C).astype(np.float32)
    comps.append((f"{name}.W_all_a", lambda w, W=W_a: _w_linear(w, W)))
    comps.append((f"{name}.W_all_b", lambda w, W=W_b: _w_linear(w, W)))
    comps.append((f"{name}.W_all_b_so", lambda w, s=scales, o=offsets: _w_scale_and_offset(w, s, o)))
    comps.append((f"{name}.lstm_nonlin", lambda w, p=params: _w_lstm_nonlinearity(w, p, False)))
    comps.append((f"{name}.cm_trunc", lambda w, n=2 * C, s=scale, i=d: _w_backprop_truncation(w, n, s, i)))
    comps.append((f"{name}.m_batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
    # (a written model holds the descriptor as nnet3 normalises it: Scale() innermost, and none where the scale is 1)
    m_trunc = f"{name}.m_trunc" if self_scale == 1.0 else f"Scale({self_scale:g}, {name}.m_trunc)"
    cfg.append(f"component-node name={name}.W_all_a component={name}.W_all_a input=Append({prev}, IfDefined(Offset({m_trunc}, {-d})))")
    cfg.append(f"component-node name={name}.W_all_b component={name}.W_all_b input={name}.W_all_a")
    cfg.append(f"component-node name={name}.W_all_b_so component={name}.W_all_b_so input={name}.W_all_b")
    cfg.append(f"component-node name={name}.lstm_nonlin component={name}.lstm_nonlin "
               f"input=Append({name}.W_all_b_so, IfDefined(Offset({name}.c_trunc, {-d})))")
    cfg.append(f"dim-range-node name={name}.m input-node={name}.lstm_nonlin dim-offset={C} dim={C}")
    cfg.append(f"component-node name={name}.cm_trunc component={name}.cm_trunc input={name}.lstm_nonlin")
    cfg.append(f"dim-range-node name={name}.c_trunc input-node={name}.cm_trunc dim-offset=0 dim={C}")
    cfg.append(f"dim-range-node name={name}.m_trunc input-node={name}.cm_trunc dim-offset={C} dim={C}")
    cfg.append(f"component-node name={name}.m_batchnorm component={name}.m_batchnorm input={name}.m")
    return f"{name}.m_batchnorm", C


def _w_ng_per_element_scale(w: KaldiWriter, scales: np.ndarray) -> None:
    # nnet-simple-component.cc:3840-3856 (NaturalGradientPerElementScaleComponent::Write), behind WriteUpdatableCommon
    _updatable_open(w, "NaturalGradientPerElementScaleComponent")
    w.token("<Params>").vector(scales).token("<IsGradient>").boolean(False)
    w.token("<Rank>").i32(8).token("<UpdatePeriod>").i32(10).token("<NumSamplesHistory>").f32(2000.0).token("<Alpha>").f32(4.0)
    w.token("</NaturalGradientPerElementScaleComponent>")


def _w_clip_gradient(w: KaldiWriter, dim: int) -> None:
    # nnet-simple-component.cc:577-600
    w.token("<ClipGradientComponent>").token("<Dim>").i32(dim).token("<ClippingThreshold>").f32(30.0)
    w.token("<NormBasedClipping>").boolean(True)
    w.token("<SelfRepairClippedProportionThreshold>").f32(0.01).token("<SelfRepairTarget>").f32(0.0).token("<SelfRepairScale>").f32(1.0)
    w.token("<NumElementsClipped>").i32(0).token("<NumElementsProcessed>").i32(0)
    w.token("<NumSelfRepaired>").i32(0).token("<NumBackpropped>").i32(0)
    w.token("</ClipGradientComponent>")


def _lstmp_block(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
                 prev: str, prev_dim: int) -> Tuple[str, int]:
    """The components and nodes XconfigLstmpLayer / XconfigLstmLayer emit (xconfig/lstm.py:440-565, 160-255), under their names.
    Returns the node the next layer reads and its dim."""
    C, R, P, out_dim = lstm_layer_dims(layer)
    d, scale = int(layer.get("delay", 3)), float(layer.get("scale", 1.0))
    scale_c, scale_r = float(layer.get("scale_c", scale)), float(layer.get("scale_r", scale))
    dropout, proj, clipgrad = bool(layer.get("dropout", False)), R > 0, bool(layer.get("clipgrad", False))
    rec_dim = R if proj else C
    if clipgrad and (scale_c != 1.0 or scale_r != 1.0):
        raise ValueError("lstm layer: a ClipGradientComponent has no scale")

    def randn(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def randb(n):
        return (rng.standard_normal(n) * 0.1).astype(np.float32)

    def affine(W, b):
        return lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)

    def trunc(n, s):
        if clipgrad:
            return lambda w, n=n: _w_clip_gradient(w, n)
        return lambda w, n=n, s=s: _w_backprop_truncation(w, n, s, d)

    for g in ("i", "f", "o"):
        W, b = np.concatenate([randn(C, prev_dim), randn(C, rec_dim)], axis=1), randb(C)
        comps.append((f"{name}.W_{g}.xr", affine(W, b)))
        comps.append((f"{name}.w_{g}.c", lambda w, v=randb(C): _w_ng_per_element_scale(w, v)))
    W, b = np.concatenate([randn(C, prev_dim), randn(C, rec_dim)], axis=1), randb(C)
    comps.append((f"{name}.W_c.xr", affine(W, b)))
    for g in ("i", "f", "o"):
        comps.append((f"{name}.{g}", lambda w: _w_nonlinear(w, "SigmoidComponent", C)))
    for g in ("g", "h"):
        comps.append((f"{name}.{g}", lambda w: _w_nonlinear(w, "TanhComponent", C)))
    if dropout:
        comps.append((f"{name}.dropout", lambda w: _w_dropout(w, C)))
    for g in ("c1", "c2", "m"):
        comps.append((f"{name}.{g}", lambda w: _w_elementwise_product(w, 2 * C, C)))
    comps.append((f"{name}.c", trunc(C, scale_c)))
    rec = f"IfDefined(Offset({name}.r_t, {-d}))"
    c_del = f"IfDefined(Offset({name}.c_t, {-d}))"
    cfg.append(f"component-node name={name}.c_t component={name}.c input=Sum({name}.c1_t, {name}.c2_t)")
    for g in ("i", "f", "o"):
        cfg.append(f"component-node name={name}.{g}1_t component={name}.W_{g}.xr input=Append({prev}, {rec})")
        cfg.append(f"component-node name={name}.{g}2_t component={name}.w_{g}.c input={c_del if g != 'o' else name + '.c_t'}")
        if dropout:
            cfg.append(f"component-node name={name}.{g}_t_predrop component={name}.{g} input=Sum({name}.{g}1_t, {name}.{g}2_t)")
            cfg.append(f"component-node name={name}.{g}_t component={name}.dropout input={name}.{g}_t_predrop")
        else:
            cfg.append(f"component-node name={name}.{g}_t component={name}.{g} input=Sum({name}.{g}1_t, {name}.{g}2_t)")
    cfg.append(f"component-node name={name}.h_t component={name}.h input={name}.c_t")
    cfg.append(f"component-node name={name}.g1_t component={name}.W_c.xr input=Append({prev}, {rec})")
    cfg.append(f"component-node name={name}.g_t component={name}.g input={name}.g1_t")
    cfg.append(f"component-node name={name}.c1_t component={name}.c1 input=Append({name}.f_t, {c_del})")
    cfg.append(f"component-node name={name}.c2_t component={name}.c2 input=Append({name}.i_t, {name}.g_t)")
    cfg.append(f"component-node name={name}.m_t component={name}.m input=Append({name}.o_t, {name}.h_t)")
    if proj:
        comps.append((f"{name}.W_rp.m", affine(randn(R + P, C), randb(R + P))))
        comps.append((f"{name}.r", trunc(R, scale_r)))
        cfg.append(f"component-node name={name}.rp_t component={name}.W_rp.m input={name}.m_t")
        cfg.append(f"dim-range-node name={name}.r_t_preclip input-node={name}.rp_t dim-offset=0 dim={R}")
        cfg.append(f"component-node name={name}.r_t component={name}.r input={name}.r_t_preclip")
        out = f"{name}.rp_t"
    else:
        comps.append((f"{name}.r", trunc(C, scale_r)))
        cfg.append(f"component-node name={name}.r_t component={name}.r input={name}.m_t")
        out = f"{name}.m_t"
    if layer.get("batchnorm", False):
        bn = out + "_batchnorm"
        mean, var = (0.1 * rng.standard_normal(out_dim)).astype(np.float32), rng.uniform(0.05, 0.2, out_dim).astype(np.float32)
        comps.append((bn, lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
        cfg.append(f"component-node name={bn} component={bn} input={out}")
        out = bn
    return out, out_dim


def _w_output_gru_nonlinearity(w: KaldiWriter, w_h: np.ndarray) -> None:
    # nnet-combined-component.cc:2204-2241 (OutputGruNonlinearityComponent::Write), behind WriteUpdatableCommon
    cell = w_h.shape[0]
    _updatable_open(w, "OutputGruNonlinearityComponent")
    w.token("<CellDim>").i32(cell).token("<w_h>").vector(w_h)
    w.token("<ValueAvg>").vector(np.zeros(cell, np.float32)).token("<DerivAvg>").vector(np.zeros(cell, np.float32))
    w.token("<SelfRepairTotal>").f64(0.0).token("<Count>").f64(0.0)
    w.token("<SelfRepairThreshold>").f32(0.2).token("<SelfRepairScale>").f32(1e-5)
    w.token("<Alpha>").f32(4.0).token("<Rank>").i32(8).token("<UpdatePeriod>").i32(10)
    w.token("</OutputGruNonlinearityComponent>")


def _w_normalize(w: KaldiWriter, dim: int, target_rms: float = 1.0, add_log_stddev: bool = False) -> None:
    # nnet-normalize-component.cc:98-111 (<BlockDim> only where it differs from the dim)
    w.token("<NormalizeComponent>").token("<InputDim>").i32(dim).token("<TargetRms>").f32(target_rms)
    w.token("<AddLogStddev>").boolean(add_log_stddev).token("</NormalizeComponent>")


def _w_dropout(w: KaldiWriter, dim: int, proportion: float = 0.0, per_frame: bool = False) -> None:
    # nnet-simple-component.cc:225-236
    w.token("<DropoutComponent>").token("<Dim>").i32(dim).token("<DropoutProportion>").f32(proportion)
    w.token("<DropoutPerFrame>").boolean(per_frame).token("<TestMode>").boolean(False).token("</DropoutComponent>")


def _w_elementwise_product(w: KaldiWriter, input_dim: int, output_dim: int) -> None:
    # nnet-simple-component.cc:312-319
    w.token("<ElementwiseProductComponent>").token("<InputDim>").i32(input_dim).token("<OutputDim>").i32(output_dim)
    w.token("</ElementwiseProductComponent>")


def _gru_form(layer: Dict[str, object]) -> str:
    form = str(layer.get("form", "fast"))
    if form not in ("fast", "composed"):
        raise ValueError("gru / pgru layer: form is 'fast' (the default) or 'composed'")
    return form


def gru_layer_dims(layer: Dict[str, object]) -> Tuple[int, int, int, int]:
    """(cell, recurrent, non-recurrent, output) dims of a ModelSpec.gru_layers entry."""
    C, R, P = int(layer["cell"]), int(layer["rec"]), int(layer["nonrec"])
    if C <= 0 or R <= 0 or P <= 0:
        raise ValueError("gru layer: cell, rec and nonrec are positive")
    if layer.get("dropout", False) and not layer.get("norm", False):
        raise ValueError("gru layer: only the norm variant has the dropout component")
    return C, R, P, R + P


def _gru_block(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
               prev: str, prev_dim: int) -> Tuple[str, int]:
    """The components and nodes XconfigFastOpgruLayer / XconfigFastNormOpgruLayer emit (xconfig/gru.py:1823-1866, 2046-2111), in
    their order.  Returns the node the next layer reads and its dim."""
    C, R, P, out_dim = gru_layer_dims(layer)
    d, scale = int(layer.get("delay", 3)), float(layer.get("scale", 1.0))
    norm, dropout = bool(layer.get("norm", False)), bool(layer.get("dropout", False))

    def randn(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def randb(n):
        return (rng.standard_normal(n) * 0.1).astype(np.float32)

    def affine(W, b):
        return lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)

    W_z, b_z = np.concatenate([randn(C, prev_dim), randn(C, R)], axis=1), randb(C)
    W_o, b_o = np.concatenate([randn(C, prev_dim), randn(C, R)], axis=1), randb(C)
    W_h, b_h = randn(C, prev_dim), randb(C)
    w_h = (rng.standard_normal(C) * 0.3).astype(np.float32)
    W_y, b_y = randn(R + P, C), randb(R + P)
    comps.append((f"{name}.W_z.xs", affine(W_z, b_z)))
    comps.append((f"{name}.W_o.xs", affine(W_o, b_o)))
    comps.append((f"{name}.W_hpart.x", affine(W_h, b_h)))
    comps.append((f"{name}.z", lambda w: _w_nonlinear(w, "SigmoidComponent", C)))
    comps.append((f"{name}.o", lambda w: _w_nonlinear(w, "SigmoidComponent", C)))
    if dropout:
        comps.append((f"{name}.dropout", lambda w: _w_dropout(w, C)))
    rec = f"IfDefined(Offset({name}.s_t, {-d}))"
    for g in ("z", "o"):
        cfg.append(f"component-node name={name}.{g}_t_pre component={name}.W_{g}.xs input=Append({prev}, {rec})")
        if dropout:
            cfg.append(f"component-node name={name}.{g}_t_predrop component={name}.{g} input={name}.{g}_t_pre")
            cfg.append(f"component-node name={name}.{g}_t component={name}.dropout input={name}.{g}_t_predrop")
        else:
            cfg.append(f"component-node name={name}.{g}_t component={name}.{g} input={name}.{g}_t_pre")
    cfg.append(f"component-node name={name}.hpart_t component={name}.W_hpart.x input={prev}")
    comps.append((f"{name}.gru_nonlin", lambda w: _w_output_gru_nonlinearity(w, w_h)))
    cfg.append(f"component-node name={name}.gru_nonlin_t component={name}.gru_nonlin "
               f"input=Append({name}.z_t, {name}.hpart_t, IfDefined(Offset({name}.c_t, {-d})))")
    cfg.append(f"dim-range-node name={name}.c_t input-node={name}.gru_nonlin_t dim-offset={C} dim={C}")
    comps.append((f"{name}.cdoto", lambda w: _w_elementwise_product(w, 2 * C, C)))
    cfg.append(f"component-node name={name}.cdoto component={name}.cdoto input=Append({name}.c_t, {name}.o_t)")
    comps.append((f"{name}.W_y.cdoto", affine(W_y, b_y)))
    y = f"{name}.y_t_tmp" if norm else f"{name}.y_t"
    cfg.append(f"component-node name={y} component={name}.W_y.cdoto input={name}.cdoto")
    if norm:
        comps.append((f"{name}.renorm", lambda w: _w_normalize(w, R)))
    comps.append((f"{name}.s_r", lambda w: _w_backprop_truncation(w, R, scale, d)))
    if norm:
        cfg.append(f"dim-range-node name={name}.s_t_pre input-node={y} dim-offset=0 dim={R}")
        cfg.append(f"component-node name={name}.s_t_renorm component={name}.renorm input={name}.s_t_pre")
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_t_renorm")
        mean, var = (0.1 * rng.standard_normal(out_dim)).astype(np.float32), rng.uniform(0.05, 0.2, out_dim).astype(np.float32)
        comps.append((f"{name}.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
        cfg.append(f"component-node name={name}.y_t component={name}.batchnorm input={y}")
    else:
        cfg.append(f"dim-range-node name={name}.s_t_preclip input-node={y} dim-offset=0 dim={R}")
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_t_preclip")
    return f"{name}.y_t", out_dim


ATTENTION_FORMS = ("attention-renorm-layer", "attention-relu-renorm-layer", "attention-relu-batchnorm-layer", "relu-renorm-attention-layer")


def attention_layer_dims(layer: Dict[str, object]) -> Tuple[int, int, int]:
    """(context positions, input dim, output dim) of a ModelSpec.attention_layers entry (attention.py:91-107)."""
    H, K, V = int(layer["heads"]), int(layer["key_dim"]), int(layer["value_dim"])
    C = int(layer["left"]) + 1 + int(layer["right"])
    return C, H * (2 * K + V + C), H * (V + (C if layer.get("output_context", True) else 0))


def attention_key_scale(layer: Dict[str, object]) -> float:
    return float(layer["key_scale"]) if "key_scale" in layer else 1.0 / math.sqrt(int(layer["key_dim"]))


def _w_attention(w: KaldiWriter, layer: Dict[str, object]) -> None:
    # nnet-attention-component.cc:442-471 (RestrictedAttentionComponent::Write); no statistics stored
    left, right = int(layer["left"]), int(layer["right"])
    left_req, right_req = int(layer.get("left_required", -1)), int(layer.get("right_required", -1))
    w.token("<RestrictedAttentionComponent>").token("<NumHeads>").i32(int(layer["heads"]))
    w.token("<KeyDim>").i32(int(layer["key_dim"])).token("<ValueDim>").i32(int(layer["value_dim"]))
    w.token("<NumLeftInputs>").i32(left).token("<NumRightInputs>").i32(right).token("<TimeStride>").i32(int(layer.get("stride", 1)))
    w.token("<NumLeftInputsRequired>").i32(left if left_req < 0 else left_req)
    w.token("<NumRightInputsRequired>").i32(right if right_req < 0 else right_req)
    w.token("<OutputContext>").boolean(bool(layer.get("output_context", True)))
    w.token("<KeyScale>").f32(attention_key_scale(layer))
    w.token("<StatsCount>").f64(0.0).token("<EntropyStats>").vector(np.zeros(0), double=True)
    w.token("<PosteriorStats>").matrix(np.zeros((0, 0)), double=True)
    w.token("</RestrictedAttentionComponent>")


def _attention_layer(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
                     prev: str, prev_dim: int) -> Tuple[str, int]:
    """The components and nodes XconfigAttentionLayer emits (xconfig/attention.py:139-249), in their order: the affine, then one node
    per word of the layer's name.  Returns the node the next layer reads and its dim."""
    form = str(layer.get("form", "attention-relu-renorm-layer"))
    if form not in ATTENTION_FORMS:
        raise ValueError(f"attention layer: form {form!r}: one of {ATTENTION_FORMS}")
    H, K, V = int(layer["heads"]), int(layer["key_dim"]), int(layer["value_dim"])
    C, in_dim, out_dim = attention_layer_dims(layer)
    W = (rng.standard_normal((in_dim, prev_dim)) / math.sqrt(prev_dim)).astype(np.float32)
    b = (rng.standard_normal(in_dim) * 0.1).astype(np.float32)
    gain = np.float32(layer.get("logit_gain", 1.0))
    if gain != 1.0:
        per_head = 2 * K + V + C
        for h in range(H):
            for lo, hi in ((0, K), (K + V, per_head)):      # the key rows, the query rows (key part and context part)
                W[h * per_head + lo:h * per_head + hi] *= gain
                b[h * per_head + lo:h * per_head + hi] *= gain
    comps.append((f"{name}.affine", lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)))
    cfg.append(f"component-node name={name}.affine component={name}.affine input={prev}")
    cur, dim = f"{name}.affine", in_dim
    for word in form.split("-")[:-1]:
        if word == "relu":
            comps.append((f"{name}.relu", lambda w, d=dim: _w_nonlinear(w, "RectifiedLinearComponent", d)))
        elif word == "attention":
            comps.append((f"{name}.attention", lambda w, l=dict(layer): _w_attention(w, l)))
            dim = out_dim
        elif word == "renorm":
            comps.append((f"{name}.renorm", lambda w, d=dim: _w_normalize(w, d)))
        else:
            mean, var = (0.1 * rng.standard_normal(dim)).astype(np.float32), rng.uniform(0.05, 0.2, dim).astype(np.float32)
            comps.append((f"{name}.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
        cfg.append(f"component-node name={name}.{word} component={name}.{word} input={cur}")
        cur = f"{name}.{word}"
    return cur, dim


def _w_gru_nonlinearity(w: KaldiWriter, w_h: np.ndarray) -> None:
    # nnet-combined-component.cc:1726-1767 (GruNonlinearityComponent::Write), behind WriteUpdatableCommon; w_h is cell x recurrent
    cell, rec = w_h.shape
    _updatable_open(w, "GruNonlinearityComponent")
    w.token("<CellDim>").i32(cell).token("<RecurrentDim>").i32(rec).token("<w_h>").matrix(w_h)
    w.token("<ValueAvg>").vector(np.zeros(cell, np.float32)).token("<DerivAvg>").vector(np.zeros(cell, np.float32))
    w.token("<SelfRepairTotal>").f64(0.0).token("<Count>").f64(0.0)
    w.token("<SelfRepairThreshold>").f32(0.2).token("<SelfRepairScale>").f32(1e-5)
    w.token("<Alpha>").f32(4.0).token("<RankInOut>").i32(8).i32(8).token("<UpdatePeriod>").i32(10)
    w.token("</GruNonlinearityComponent>")


def pgru_layer_dims(layer: Dict[str, object]) -> Tuple[int, int, int, int]:
    """(cell, recurrent, non-recurrent, output) dims of a ModelSpec.pgru_layers entry; without a projection (rec = nonrec = 0) the
    recurrent and the output dim are the cell dim."""
    C, R, P = int(layer["cell"]), int(layer.get("rec", 0)), int(layer.get("nonrec", 0))
    if C <= 0 or R < 0 or P < 0 or (R == 0) != (P == 0):
        raise ValueError("pgru layer: cell is positive; rec and nonrec are both positive or both 0 (fast-gru-layer)")
    if layer.get("norm", False) and R == 0:
        raise ValueError("pgru layer: there is no norm variant of fast-gru-layer")
    if layer.get("dropout", False) and not layer.get("norm", False):
        raise ValueError("pgru layer: only the norm variant has the dropout components")
    return (C, R, P, R + P) if R > 0 else (C, C, 0, C)


def _pgru_block(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
                prev: str, prev_dim: int) -> Tuple[str, int]:
    """The components and nodes XconfigFastGruLayer / XconfigFastPgruLayer / XconfigFastNormPgruLayer emit (xconfig/gru.py:1160-1197,
    1367-1407, 1587-1653), in their order.  Returns the node the next layer reads and its dim."""
    C, R, P, out_dim = pgru_layer_dims(layer)
    proj = int(layer.get("rec", 0)) > 0
    d, scale = int(layer.get("delay", 3)), float(layer.get("scale", 1.0))
    norm, dropout = bool(layer.get("norm", False)), bool(layer.get("dropout", False))
    xs = "xs" if proj else "xh"

    def randn(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def randb(n):
        return (rng.standard_normal(n) * 0.1).astype(np.float32)

    def affine(W, b):
        return lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)

    W_z, b_z = np.concatenate([randn(C, prev_dim), randn(C, R)], axis=1), randb(C)
    W_r, b_r = np.concatenate([randn(R, prev_dim), randn(R, R)], axis=1), randb(R)
    W_hp, b_hp = randn(C, prev_dim), randb(C)
    w_h = randn(C, R)
    comps.append((f"{name}.W_z.{xs}", affine(W_z, b_z)))
    comps.append((f"{name}.W_r.{xs}", affine(W_r, b_r)))
    comps.append((f"{name}.W_hpart.x", affine(W_hp, b_hp)))
    comps.append((f"{name}.z", lambda w: _w_nonlinear(w, "SigmoidComponent", C)))
    comps.append((f"{name}.r", lambda w: _w_nonlinear(w, "SigmoidComponent", R)))
    if dropout:
        comps.append((f"{name}.dropout_z", lambda w: _w_dropout(w, C)))
        comps.append((f"{name}.dropout_r", lambda w: _w_dropout(w, R)))
    rec = f"IfDefined(Offset({name}.s_t, {-d}))"
    for g in ("z", "r"):
        cfg.append(f"component-node name={name}.{g}_t_pre component={name}.W_{g}.{xs} input=Append({prev}, {rec})")
        if dropout:
            cfg.append(f"component-node name={name}.{g}_t_predrop component={name}.{g} input={name}.{g}_t_pre")
            cfg.append(f"component-node name={name}.{g}_t component={name}.dropout_{g} input={name}.{g}_t_predrop")
        else:
            cfg.append(f"component-node name={name}.{g}_t component={name}.{g} input={name}.{g}_t_pre")
    cfg.append(f"component-node name={name}.hpart_t component={name}.W_hpart.x input={prev}")
    comps.append((f"{name}.gru_nonlin", lambda w: _w_gru_nonlinearity(w, w_h)))
    if not proj:
        cfg.append(f"component-node name={name}.gru_nonlin_t component={name}.gru_nonlin "
                   f"input=Append({name}.z_t, {name}.r_t, {name}.hpart_t, {rec})")
        cfg.append(f"dim-range-node name={name}.y_t input-node={name}.gru_nonlin_t dim-offset={C} dim={C}")
        comps.append((f"{name}.s_r", lambda w: _w_backprop_truncation(w, C, scale, d)))
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.y_t")
        return f"{name}.y_t", out_dim
    cfg.append(f"component-node name={name}.gru_nonlin_t component={name}.gru_nonlin "
               f"input=Append({name}.z_t, {name}.r_t, {name}.hpart_t, IfDefined(Offset({name}.c_t, {-d})), {rec})")
    cfg.append(f"dim-range-node name={name}.c_t input-node={name}.gru_nonlin_t dim-offset={C} dim={C}")
    W_y, b_y = randn(R + P, C), randb(R + P)
    comps.append((f"{name}.W_y.c", affine(W_y, b_y)))
    y = f"{name}.y_t_tmp" if norm else f"{name}.y_t"
    cfg.append(f"component-node name={y} component={name}.W_y.c input={name}.c_t")
    if norm:
        comps.append((f"{name}.renorm", lambda w: _w_normalize(w, R)))
    comps.append((f"{name}.s_r", lambda w: _w_backprop_truncation(w, R, scale, d)))
    cfg.append(f"dim-range-node name={name}.s_t_pre input-node={y} dim-offset=0 dim={R}")
    if norm:
        cfg.append(f"component-node name={name}.s_t_renorm component={name}.renorm input={name}.s_t_pre")
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_t_renorm")
        mean, var = (0.1 * rng.standard_normal(out_dim)).astype(np.float32), rng.uniform(0.05, 0.2, out_dim).astype(np.float32)
        comps.append((f"{name}.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
        cfg.append(f"component-node name={name}.y_t component={name}.batchnorm input={y}")
    else:
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_t_pre")
    return f"{name}.y_t", out_dim


def _gruc_block(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
                prev: str, prev_dim: int) -> Tuple[str, int]:
    """A gru_layers entry with form="composed": the components and nodes XconfigOpgruLayer / XconfigNormOpgruLayer emit
    (xconfig/gru.py:754-806, 972-1042), in their order and under their names.  Returns the node the next layer reads and its dim."""
    C, R, P, out_dim = gru_layer_dims(layer)
    d, scale = int(layer.get("delay", 3)), float(layer.get("scale", 1.0))
    norm, dropout = bool(layer.get("norm", False)), bool(layer.get("dropout", False))

    def randn(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def randb(n):
        return (rng.standard_normal(n) * 0.1).astype(np.float32)

    def affine(W, b):
        return lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)

    for g in ("z", "o"):
        comps.append((f"{name}.W_z.xs_{g}", affine(np.concatenate([randn(C, prev_dim), randn(C, R)], axis=1), randb(C))))
    comps.append((f"{name}.W_h.UW", affine(randn(C, prev_dim), randb(C))))
    comps.append((f"{name}.W_h.UW_elementwise", lambda w, v=(rng.standard_normal(C) * 0.3).astype(np.float32): _w_ng_per_element_scale(w, v)))
    for g in ("z", "o"):
        comps.append((f"{name}.{g}", lambda w: _w_nonlinear(w, "SigmoidComponent", C)))
    comps.append((f"{name}.h", lambda w: _w_nonlinear(w, "TanhComponent", C)))
    for g in ("o1", "y1", "y2"):
        comps.append((f"{name}.{g}", lambda w: _w_elementwise_product(w, 2 * C, C)))
    comps.append((f"{name}.y", lambda w: _w_noop(w, C)))
    if dropout:
        comps.append((f"{name}.dropout", lambda w: _w_dropout(w, C)))
    rec, rec_y = f"IfDefined(Offset({name}.s_t, {-d}))", f"IfDefined(Offset({name}.y_t, {-d}))"
    for g in ("z", "o"):
        cfg.append(f"component-node name={name}.{g}_t_pre component={name}.W_z.xs_{g} input=Append({prev}, {rec})")
        if dropout:
            cfg.append(f"component-node name={name}.{g}_predrop_t component={name}.{g} input={name}.{g}_t_pre")
            cfg.append(f"component-node name={name}.{g}_t component={name}.dropout input={name}.{g}_predrop_t")
        else:
            cfg.append(f"component-node name={name}.{g}_t component={name}.{g} input={name}.{g}_t_pre")
    cfg.append(f"component-node name={name}.h_t_pre component={name}.W_h.UW input={prev}")
    cfg.append(f"component-node name={name}.h_t_pre2 component={name}.W_h.UW_elementwise input={rec_y}")
    cfg.append(f"component-node name={name}.h_t component={name}.h input=Sum({name}.h_t_pre, {name}.h_t_pre2)")
    cfg.append(f"component-node name={name}.y1_t component={name}.y1 input=Append({name}.h_t, Sum(Scale(-1, {name}.z_t), Const(1, {C})))")
    cfg.append(f"component-node name={name}.y2_t component={name}.y2 input=Append({rec_y}, {name}.z_t)")
    cfg.append(f"component-node name={name}.y_t component={name}.y input=Sum({name}.y1_t, {name}.y2_t)")
    cfg.append(f"component-node name={name}.y_o_t component={name}.o1 input=Append({name}.o_t, {name}.y_t)")
    comps.append((f"{name}.W_s.ys", affine(randn(R + P, C), randb(R + P))))
    comps.append((f"{name}.s_r", lambda w: _w_backprop_truncation(w, R, scale, d)))
    if not norm:
        cfg.append(f"component-node name={name}.sn_t component={name}.W_s.ys input={name}.y_o_t")
        cfg.append(f"dim-range-node name={name}.s_t_preclip input-node={name}.sn_t dim-offset=0 dim={R}")
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_t_preclip")
        return f"{name}.sn_t", out_dim
    mean, var = (0.1 * rng.standard_normal(out_dim)).astype(np.float32), rng.uniform(0.05, 0.2, out_dim).astype(np.float32)
    comps.append((f"{name}.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
    comps.append((f"{name}.renorm", lambda w: _w_normalize(w, R)))
    cfg.append(f"component-node name={name}.sn_nobatchnorm_t component={name}.W_s.ys input={name}.y_o_t")
    cfg.append(f"component-node name={name}.sn_t component={name}.batchnorm input={name}.sn_nobatchnorm_t")
    cfg.append(f"dim-range-node name={name}.s_t_preclip input-node={name}.sn_nobatchnorm_t dim-offset=0 dim={R}")
    cfg.append(f"component-node name={name}.s_t_preclip_renorm component={name}.renorm input={name}.s_t_preclip")
    cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_t_preclip_renorm")
    return f"{name}.sn_t", out_dim


def _pgruc_block(cfg: List[str], comps: List[Tuple[str, object]], rng: np.random.Generator, name: str, layer: Dict[str, object],
                 prev: str, prev_dim: int) -> Tuple[str, int]:
    """A pgru_layers entry with form="composed": the components and nodes XconfigGruLayer (rec = nonrec = 0) / XconfigPgruLayer /
    XconfigNormPgruLayer emit (xconfig/gru.py:122-169, 320-371, 533-605), in their order and under their names.  Returns the node the
    next layer reads and its dim."""
    C, R, P, out_dim = pgru_layer_dims(layer)
    proj = int(layer.get("rec", 0)) > 0
    d, scale = int(layer.get("delay", 3)), float(layer.get("scale", 1.0))
    norm, dropout = bool(layer.get("norm", False)), bool(layer.get("dropout", False))

    def randn(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def randb(n):
        return (rng.standard_normal(n) * 0.1).astype(np.float32)

    def affine(W, b):
        return lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)

    for g, rows in (("z", C), ("r", R)):
        comps.append((f"{name}.W_z.xs_{g}", affine(np.concatenate([randn(rows, prev_dim), randn(rows, R)], axis=1), randb(rows))))
    comps.append((f"{name}.W_h.UW", affine(np.concatenate([randn(C, prev_dim), randn(C, R)], axis=1), randb(C))))
    if dropout:
        comps.append((f"{name}.dropout_z", lambda w: _w_dropout(w, C)))
        comps.append((f"{name}.dropout_r", lambda w: _w_dropout(w, R)))
    comps.append((f"{name}.z", lambda w: _w_nonlinear(w, "SigmoidComponent", C)))
    comps.append((f"{name}.r", lambda w: _w_nonlinear(w, "SigmoidComponent", R)))
    comps.append((f"{name}.h", lambda w: _w_nonlinear(w, "TanhComponent", C)))
    comps.append((f"{name}.h1", lambda w: _w_elementwise_product(w, 2 * R, R)))
    comps.append((f"{name}.y1", lambda w: _w_elementwise_product(w, 2 * C, C)))
    comps.append((f"{name}.y2", lambda w: _w_elementwise_product(w, 2 * C, C)))
    comps.append((f"{name}.y", lambda w: _w_noop(w, C)))
    rec = f"IfDefined(Offset({name}.s_t, {-d}))"
    rec_y = f"IfDefined(Offset({name}.y_t, {-d}))" if proj else rec
    for g in ("z", "r"):
        cfg.append(f"component-node name={name}.{g}_t_pre component={name}.W_z.xs_{g} input=Append({prev}, {rec})")
        if dropout:
            cfg.append(f"component-node name={name}.{g}_predrop_t component={name}.{g} input={name}.{g}_t_pre")
            cfg.append(f"component-node name={name}.{g}_t component={name}.dropout_{g} input={name}.{g}_predrop_t")
        else:
            cfg.append(f"component-node name={name}.{g}_t component={name}.{g} input={name}.{g}_t_pre")
    cfg.append(f"component-node name={name}.h1_t component={name}.h1 input=Append({name}.r_t, {rec})")
    cfg.append(f"component-node name={name}.h_t_pre component={name}.W_h.UW input=Append({prev}, {name}.h1_t)")
    cfg.append(f"component-node name={name}.h_t component={name}.h input={name}.h_t_pre")
    cfg.append(f"component-node name={name}.y1_t component={name}.y1 input=Append({name}.h_t, Sum(Scale(-1, {name}.z_t), Const(1, {C})))")
    cfg.append(f"component-node name={name}.y2_t component={name}.y2 input=Append({rec_y}, {name}.z_t)")
    cfg.append(f"component-node name={name}.y_t component={name}.y input=Sum({name}.y1_t, {name}.y2_t)")
    if not proj:
        comps.append((f"{name}.s_r", lambda w: _w_backprop_truncation(w, C, scale, d)))
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.y_t")
        return f"{name}.s_t", out_dim
    comps.append((f"{name}.W_s.ys", affine(randn(R + P, C), randb(R + P))))
    comps.append((f"{name}.s_r", lambda w: _w_backprop_truncation(w, R, scale, d)))
    if not norm:
        cfg.append(f"component-node name={name}.sn_t component={name}.W_s.ys input={name}.y_t")
        cfg.append(f"dim-range-node name={name}.s_t_preclip input-node={name}.sn_t dim-offset=0 dim={R}")
        cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_t_preclip")
        return f"{name}.sn_t", out_dim
    mean, var = (0.1 * rng.standard_normal(out_dim)).astype(np.float32), rng.uniform(0.05, 0.2, out_dim).astype(np.float32)
    comps.append((f"{name}.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
    comps.append((f"{name}.renorm", lambda w: _w_normalize(w, R)))
    cfg.append(f"component-node name={name}.sn_nobatchnorm_t component={name}.W_s.ys input={name}.y_t")
    cfg.append(f"dim-range-node name={name}.s_t_preclip input-node={name}.sn_nobatchnorm_t dim-offset=0 dim={R}")
    cfg.append(f"component-node name={name}.sn_t component={name}.batchnorm input={name}.sn_nobatchnorm_t")
    cfg.append(f"component-node name={name}.s_renorm_t component={name}.renorm input={name}.s_t_preclip")
    cfg.append(f"component-node name={name}.s_t component={name}.s_r input={name}.s_renorm_t")
    return f"{name}.sn_t", out_dim


def _append_desc(src: str, offsets: Sequence[int]) -> str:
    parts = [src if o == 0 else f"Offset({src}, {o})" for o in offsets]
    return parts[0] if len(parts) == 1 else "Append(" + ", ".join(parts) + ")"


def build_nnet(spec: ModelSpec, rng: np.random.Generator):
    """Returns (config_lines, [(name, writer_fn)], params dict for the numpy oracle)."""
    cfg: List[str] = []
    comps: List[Tuple[str, object]] = []
    C, D = spec.feat_dim, spec.ivector_dim
    cfg.append(f"input-node name=input dim={C}")
    if D > 0:
        cfg.append(f"input-node name=ivector dim={D}")

    def randw(o, i):
        if spec.weight_dist == "heavy":
            return np.clip(rng.standard_t(2.0, (o, i)) / math.sqrt(i), -1000.0, 1000.0).astype(np.float32)
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def randb(o, s=0.1):
        return (rng.standard_normal(o) * s).astype(np.float32)

    # the convolutional front end, if any: [idct + batchnorm] [iVector maps, combined] conv-relu-batchnorm layers
    front, front_dim, scaled, iv_direct = "input", C, False, D > 0
    if spec.conv_layers:
        height, filters = C, 1
        if spec.conv_idct:
            Wi = randw(C, C) * np.float32(spec.input_scale)
            comps.append(("idct", lambda w, W=Wi, b=np.zeros(C, np.float32): _w_fixed_affine(w, W, b)))
            cfg.append("component-node name=idct component=idct input=input")
            mean, var = (0.1 * rng.standard_normal(C)).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32)
            comps.append(("idct.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
            cfg.append("component-node name=idct.batchnorm component=idct.batchnorm input=idct")
            front, scaled = "idct.batchnorm", True
        if spec.conv_ivector_maps > 0:
            if D <= 0:
                raise ValueError("conv_ivector_maps needs an iVector extractor")
            M = spec.conv_ivector_maps
            comps.append(("ivector-linear", lambda w, W=randw(M * height, D): _w_linear(w, W)))
            cfg.append("component-node name=ivector-linear component=ivector-linear input=ReplaceIndex(ivector, t, 0)")
            mean, var = (0.1 * rng.standard_normal(M * height)).astype(np.float32), rng.uniform(0.5, 1.5, M * height).astype(np.float32)
            comps.append(("ivector-batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
            cfg.append("component-node name=ivector-batchnorm component=ivector-batchnorm input=ivector-linear")
            comps.append(("combine-inputs", lambda w, cm=combine_feature_maps(height, filters, M): _w_permute(w, cm)))
            cfg.append(f"component-node name=combine-inputs component=combine-inputs input=Append({front}, ivector-batchnorm)")
            front, filters, iv_direct = "combine-inputs", filters + M, False
        for ci, layer in enumerate(spec.conv_layers, start=1):
            offs = conv_layer_offsets(layer)
            f_out, h_out, sub = int(layer["filters"]), int(layer["height_out"]), int(layer.get("sub", 1))
            required = sorted(set(int(t) for t in layer.get("required_time_offsets", [t for t, _ in offs])))
            Wc, bc = randw(f_out, len(offs) * filters) * np.float32(layer.get("gain", 1.0)), randb(f_out)
            if not scaled:
                Wc, scaled = Wc * np.float32(spec.input_scale), True
            comps.append((f"cnn{ci}.conv", lambda w, a=(filters, f_out, height, h_out, sub, offs, required, Wc, bc): _w_conv(w, *a)))
            cfg.append(f"component-node name=cnn{ci}.conv component=cnn{ci}.conv input={front}")
            comps.append((f"cnn{ci}.relu", lambda w, d=f_out * h_out: _w_nonlinear(w, "RectifiedLinearComponent", d)))
            cfg.append(f"component-node name=cnn{ci}.relu component=cnn{ci}.relu input=cnn{ci}.conv")
            mean, var = (0.4 + 0.1 * rng.standard_normal(f_out)).astype(np.float32), rng.uniform(0.5, 1.5, f_out).astype(np.float32)
            comps.append((f"cnn{ci}.batchnorm", lambda w, m=mean, v=var, d=f_out * h_out: _w_batchnorm(w, m, v, dim=d)))
            cfg.append(f"component-node name=cnn{ci}.batchnorm component=cnn{ci}.batchnorm input=cnn{ci}.relu")
            front, filters, height = f"cnn{ci}.batchnorm", f_out, h_out
        front_dim = filters * height

    # lda
    lda_in = front_dim * len(spec.lda_offsets) + (D if iv_direct else 0)
    parts = [(front if o == 0 else f"Offset({front}, {o})") for o in spec.lda_offsets]
    if iv_direct:
        parts.append("ReplaceIndex(ivector, t, 0)")
    lda_desc = "Append(" + ", ".join(parts) + ")" if len(parts) > 1 else parts[0]
    if spec.conv_layers:      # (not square: the stack's output can be thousands of columns wide)
        Wl, bl = randw(spec.hidden_dim, lda_in), randb(spec.hidden_dim)
        lda_in = spec.hidden_dim
    else:
        Wl, bl = randw(lda_in, lda_in), randb(lda_in)
        Wl[:, :C * len(spec.lda_offsets)] *= np.float32(spec.input_scale)
    comps.append(("lda", lambda w, W=Wl, b=bl: _w_fixed_affine(w, W, b)))
    cfg.append(f"component-node name=lda component=lda input={lda_desc}")
    prev, prev_dim = "lda", lda_in

    def lstm_blocks_after(n_layers, prev, prev_dim):
        for k, layer in enumerate(spec.lstm_layers, start=1):
            if int(layer["after"]) == n_layers:
                prev, prev_dim = _lstm_block(cfg, comps, rng, f"lstm{k}", layer, prev, prev_dim)
        for k, layer in enumerate(spec.gru_layers, start=1):
            if int(layer["after"]) == n_layers:
                prev, prev_dim = (_gruc_block if _gru_form(layer) == "composed" else _gru_block)(cfg, comps, rng, f"gru{k}", layer, prev, prev_dim)
        for k, layer in enumerate(spec.pgru_layers, start=1):
            if int(layer["after"]) == n_layers:
                prev, prev_dim = (_pgruc_block if _gru_form(layer) == "composed" else _pgru_block)(cfg, comps, rng, f"pgru{k}", layer, prev, prev_dim)
        for k, layer in enumerate(spec.attention_layers, start=1):
            if int(layer["after"]) == n_layers:
                prev, prev_dim = _attention_layer(cfg, comps, rng, f"attention{k}", layer, prev, prev_dim)
        for k, layer in enumerate(spec.scale_offset_layers, start=1):
            if int(layer["after"]) == n_layers:
                block = int(layer.get("block", prev_dim))
                if block <= 0 or prev_dim % block != 0:
                    raise ValueError("scale-offset layer: the layer's dim is a multiple of 'block'")
                sc, of = rng.uniform(0.5, 1.5, block).astype(np.float32), (rng.standard_normal(block) * 0.1).astype(np.float32)
                comps.append((f"so{k}", lambda w, s=sc, o=of, n=prev_dim: _w_scale_and_offset(w, s, o, n)))
                cfg.append(f"component-node name=so{k} component=so{k} input={prev}")
                prev = f"so{k}"
        return prev, prev_dim

    for layer in spec.lstm_layers:
        if not 1 <= int(layer["after"]) <= len(spec.layer_offsets):
            raise ValueError("lstm layer: 'after' counts the TDNN layers in front of the block, 1 .. len(layer_offsets)")
    for layer in spec.gru_layers:
        if not 1 <= int(layer["after"]) <= len(spec.layer_offsets):
            raise ValueError("gru layer: 'after' counts the TDNN layers in front of the block, 1 .. len(layer_offsets)")
    for layer in spec.pgru_layers:
        if not 1 <= int(layer["after"]) <= len(spec.layer_offsets):
            raise ValueError("pgru layer: 'after' counts the TDNN layers in front of the block, 1 .. len(layer_offsets)")
    for layer in spec.scale_offset_layers:
        if not 1 <= int(layer["after"]) <= len(spec.layer_offsets):
            raise ValueError("scale-offset layer: 'after' counts the TDNN layers in front of the component, 1 .. len(layer_offsets)")
    for layer in spec.attention_layers:
        if not 1 <= int(layer["after"]) <= len(spec.layer_offsets):
            raise ValueError("attention layer: 'after' counts the TDNN layers in front of the layer, 1 .. len(layer_offsets)")
    for li, offs in enumerate(spec.layer_offsets, start=1):
        H = spec.hidden_dim
        prev, prev_dim = lstm_blocks_after(li - 1, prev, prev_dim)
        if spec.tdnnf and li > 1:
            # factorized layer: linear bottleneck (TdnnComponent w/o bias) -> affine (TdnnComponent) -> relu -> bn
            # -> dropout(test: identity) -> Sum(Scale(0.66, prev), this) residual through NoOp
            lo = [o for o in offs if o <= 0]
            ro = [o for o in offs if o >= 0]
            B = spec.bottleneck_dim
            W1 = randw(B, prev_dim * len(lo))
            comps.append((f"tdnnf{li}.linear", lambda w, o=lo, W=W1: _w_tdnn(w, o, W, None)))
            cfg.append(f"component-node name=tdnnf{li}.linear component=tdnnf{li}.linear input={prev}")
            W2, b2 = randw(H, B * len(ro)), randb(H)
            comps.append((f"tdnnf{li}.affine", lambda w, o=ro, W=W2, b=b2: _w_tdnn(w, o, W, b)))
            cfg.append(f"component-node name=tdnnf{li}.affine component=tdnnf{li}.affine input=tdnnf{li}.linear")
            comps.append((f"tdnnf{li}.relu", lambda w, d=H: _w_nonlinear(w, "RectifiedLinearComponent", d)))
            cfg.append(f"component-node name=tdnnf{li}.relu component=tdnnf{li}.relu input=tdnnf{li}.affine")
            mean, var = (0.4 + 0.1 * rng.standard_normal(H)).astype(np.float32), rng.uniform(0.1, 0.5, H).astype(np.float32)
            comps.append((f"tdnnf{li}.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
            cfg.append(f"component-node name=tdnnf{li}.batchnorm component=tdnnf{li}.batchnorm input=tdnnf{li}.relu")
            comps.append((f"tdnnf{li}.dropout", lambda w, d=H: _w_general_dropout(w, d)))
            cfg.append(f"component-node name=tdnnf{li}.dropout component=tdnnf{li}.dropout input=tdnnf{li}.batchnorm")
            comps.append((f"tdnnf{li}.noop", lambda w, d=H: _w_noop(w, d)))
            if prev_dim == H:
                cfg.append(f"component-node name=tdnnf{li}.noop component=tdnnf{li}.noop "
                           f"input=Sum(Scale(0.66, {prev}), tdnnf{li}.dropout)")
            else:
                cfg.append(f"component-node name=tdnnf{li}.noop component=tdnnf{li}.noop input=tdnnf{li}.dropout")
            prev, prev_dim = f"tdnnf{li}.noop", H
            continue
        W, b = randw(H, prev_dim * len(offs)), randb(H)
        if li == 2 and spec.hidden_gain != 1.0:
            W = (W * np.float32(spec.hidden_gain)).astype(np.float32)
            if spec.gain_compensated:
                b = (b * np.float32(spec.hidden_gain)).astype(np.float32)
        if li == 3 and spec.hidden_gain != 1.0 and spec.gain_compensated:
            W = (W / np.float32(spec.hidden_gain)).astype(np.float32)
        comps.append((f"tdnn{li}.affine", lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)))
        cfg.append(f"component-node name=tdnn{li}.affine component=tdnn{li}.affine input={_append_desc(prev, offs)}")
        comps.append((f"tdnn{li}.relu", lambda w, d=H: _w_nonlinear(w, "RectifiedLinearComponent", d)))
        cfg.append(f"component-node name=tdnn{li}.relu component=tdnn{li}.relu input=tdnn{li}.affine")
        if li == 2 and spec.gain_compensated:
            prev, prev_dim = f"tdnn{li}.relu", H
            continue
        mean, var = (0.4 + 0.1 * rng.standard_normal(H)).astype(np.float32), rng.uniform(0.1, 0.5, H).astype(np.float32)
        comps.append((f"tdnn{li}.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
        cfg.append(f"component-node name=tdnn{li}.batchnorm component=tdnn{li}.batchnorm input=tdnn{li}.relu")
        prev, prev_dim = f"tdnn{li}.batchnorm", H

    prev, prev_dim = lstm_blocks_after(len(spec.layer_offsets), prev, prev_dim)
    # prefinal-chain: affine -> relu -> batchnorm
    Pd = spec.prefinal_dim
    W, b = randw(Pd, prev_dim), randb(Pd)
    comps.append(("prefinal-chain.affine", lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)))
    cfg.append(f"component-node name=prefinal-chain.affine component=prefinal-chain.affine input={prev}")
    comps.append(("prefinal-chain.relu", lambda w, d=Pd: _w_nonlinear(w, "RectifiedLinearComponent", d)))
    cfg.append("component-node name=prefinal-chain.relu component=prefinal-chain.relu input=prefinal-chain.affine")
    mean, var = (0.4 + 0.1 * rng.standard_normal(Pd)).astype(np.float32), rng.uniform(0.1, 0.5, Pd).astype(np.float32)
    comps.append(("prefinal-chain.batchnorm", lambda w, m=mean, v=var: _w_batchnorm(w, m, v)))
    cfg.append("component-node name=prefinal-chain.batchnorm component=prefinal-chain.batchnorm input=prefinal-chain.relu")
    P = spec.num_pdfs
    W, b = randw(P, Pd) * np.float32(spec.output_scale), randb(P, 0.5)
    comps.append(("output.affine", lambda w, W=W, b=b: _w_affine(w, "NaturalGradientAffineComponent", W, b)))
    cfg.append("component-node name=output.affine component=output.affine input=prefinal-chain.batchnorm")
    out_src = "output.affine"
    if spec.with_log_softmax:
        comps.append(("output.log-softmax", lambda w, d=P: _w_nonlinear(w, "LogSoftmaxComponent", d)))
        cfg.append("component-node name=output.log-softmax component=output.log-softmax input=output.affine")
        out_src = "output.log-softmax"
    cfg.append(f"output-node name=output input={out_src} objective=linear")
    if spec.xent_branch:
        # chain recipes carry a second (xent) output; it must be ignored by decoding
        Wx, bx = randw(P, prev_dim), randb(P)
        comps.append(("output-xent.affine", lambda w, W=Wx, b=bx: _w_affine(w, "NaturalGradientAffineComponent", W, b)))
        cfg.append(f"component-node name=output-xent.affine component=output-xent.affine input={prev}")
        comps.append(("output-xent.log-softmax", lambda w, d=P: _w_nonlinear(w, "LogSoftmaxComponent", d)))
        cfg.append("component-node name=output-xent.log-softmax component=output-xent.log-softmax input=output-xent.affine")
        cfg.append("output-node name=output-xent input=output-xent.log-softmax objective=linear")
    return cfg, comps


def write_final_mdl(path: Path, spec: ModelSpec, nnet=None) -> None:
    """nnet: None for the network of build_nnet(spec), or (config lines, [(component name, writer_fn)]) of a network written by
    hand: its input-node dims are spec.feat_dim and spec.ivector_dim, its output dim spec.num_pdfs; transition model, priors,
    extractor, tree and graph are the spec's either way."""
    rng = np.random.default_rng(spec.seed)
    w = KaldiWriter(spec.binary)
    _write_transition_model(w, spec)
    cfg, comps = build_nnet(spec, rng) if nnet is None else nnet
    w.token("<Nnet3>").raw(b"\n")
    w.raw(("\n".join(cfg) + "\n\n").encode())
    w.token("<NumComponents>").i32(len(comps)).nl()
    for name, fn in comps:
        w.token("<ComponentName>").token(name)
        fn(w)
        w.nl()
    w.token("</Nnet3>").nl()
    w.token("<LeftContext>").i32(0).token("<RightContext>").i32(0)   # recomputed by the reader (am-nnet-simple.cc:52)
    w.token("<Priors>")
    if spec.with_priors:
        pri = rng.uniform(0.2, 1.0, spec.num_pdfs)
        w.vector((pri / pri.sum()).astype(np.float32))
    else:
        w.vector(np.zeros(0, np.float32))
    w.nl()
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(w.getvalue())


# --------------------------------------------------------------------------- iVector extractor + confs


def write_ivector_extractor(ie_dir: Path, spec: ModelSpec) -> None:
    rng = np.random.default_rng(spec.seed + 7919)
    ie_dir.mkdir(parents=True, exist_ok=True)
    C, Dl, G, Di = spec.feat_dim, spec.lda_dim, spec.num_gauss, spec.ivector_dim
    nsp = spec.splice_left + 1 + spec.splice_right
    # final.mat: affine LDA, D_lda x (C*nsp + 1); scaled so outputs are O(1) for MFCC-sized inputs
    lda = (rng.standard_normal((Dl, C * nsp + 1)) * (0.05 / math.sqrt(C * nsp))).astype(np.float32)
    lda[:, -1] = (rng.standard_normal(Dl) * 0.1).astype(np.float32)
    write_kaldi_matrix_file(ie_dir / "final.mat", lda, spec.binary)
    # global_cmvn.stats: 2 x (C+1) double: sums, sumsq; count in [0][C]
    cnt = 10000.0
    mean = rng.standard_normal(C) * 2.0
    mean[0] += 60.0
    stats = np.zeros((2, C + 1))
    stats[0, :C] = mean * cnt
    stats[0, C] = cnt
    stats[1, :C] = (mean * mean + 25.0) * cnt
    write_kaldi_matrix_file(ie_dir / "global_cmvn.stats", stats, spec.binary, double=True)
    # final.dubm
    means = rng.standard_normal((G, Dl)) * 1.0
    inv_vars = 1.0 / rng.uniform(0.5, 2.0, (G, Dl))
    weights = rng.uniform(0.5, 1.5, G)
    weights /= weights.sum()
    w = KaldiWriter(spec.binary)
    w.token("<DiagGMM>").nl()
    gconsts = np.log(weights) - 0.5 * math.log(2 * math.pi) * Dl + 0.5 * np.log(inv_vars).sum(1) \
        - 0.5 * (means * means * inv_vars).sum(1)
    w.token("<GCONSTS>").vector(gconsts.astype(np.float32))
    w.token("<WEIGHTS>").vector(weights.astype(np.float32))
    w.token("<MEANS_INVVARS>").matrix((means * inv_vars).astype(np.float32))
    w.token("<INV_VARS>").matrix(inv_vars.astype(np.float32))
    w.token("</DiagGMM>").nl()
    (ie_dir / "final.dubm").write_bytes(w.getvalue())
    # final.ie
    w = KaldiWriter(spec.binary)
    w.token("<IvectorExtractor>")
    w.token("<w>").matrix(np.zeros((0, 0)), double=True)
    w.token("<w_vec>").vector(np.log(weights), double=True)
    w.token("<M>").i32(G)
    for g in range(G):
        M = rng.standard_normal((Dl, Di)) * 0.3
        M[:, 0] = means[g] / 5.0          # first column carries the (offset-scaled) mean, as in trained extractors
        w.matrix(M, double=True)
    w.token("<SigmaInv>")
    for g in range(G):
        A = rng.standard_normal((Dl, Dl)) * 0.1
        S = A @ A.T + np.diag(rng.uniform(0.5, 2.0, Dl))
        w.sp_matrix(S, double=True)
    w.token("<IvectorOffset>").f64(5.0)
    w.token("</IvectorExtractor>")
    (ie_dir / "final.ie").write_bytes(w.getvalue())


def write_model_dir(model_dir: Path, spec: ModelSpec, nnet=None) -> None:
    """Writes <model_dir>/model/{model,online} in the layout of SURVEY.md §3.4.  nnet: as write_final_mdl's."""
    model_dir = Path(model_dir).absolute()
    write_final_mdl(model_dir / "model" / "model" / "final.mdl", spec, nnet)
    write_tree(model_dir / "model" / "model" / "tree", spec)
    conf = model_dir / "model" / "online" / "conf"
    conf.mkdir(parents=True, exist_ok=True)
    low_freq = 20 if spec.low_freq is None else spec.low_freq
    high_freq = -400 if spec.high_freq is None else spec.high_freq
    if spec.feature_type == "mfcc" and spec.mfcc_defaults:
        if (spec.num_mel_bins, spec.num_ceps) != (23, 13):
            raise ValueError("mfcc_defaults: the reference's defaults are 23 mel bins and 13 cepstra")
        (conf / "mfcc.conf").write_text(f"--sample-frequency={spec.sample_frequency}\n--use-energy=false\n")
        online = ["--feature-type=mfcc", f"--mfcc-config={conf / 'mfcc.conf'}"]
    elif spec.feature_type == "mfcc":
        mfcc = ["--use-energy=false", f"--num-mel-bins={spec.num_mel_bins}", f"--num-ceps={spec.num_ceps}",
                f"--low-freq={low_freq}", f"--high-freq={high_freq}", f"--sample-frequency={spec.sample_frequency}"]
        if spec.dither is not None:
            mfcc.append(f"--dither={spec.dither}")
        if spec.frame_length is not None:
            mfcc.append(f"--frame-length={spec.frame_length}")
        (conf / "mfcc.conf").write_text("# hires MFCC (egs/wsj/s5/conf/mfcc_hires.conf)\n" + "\n".join(mfcc) + "\n")
        online = ["--feature-type=mfcc", f"--mfcc-config={conf / 'mfcc.conf'}"]
    else:
        _ = spec.feat_dim      # (refuses a type other than fbank)
        online = ["--feature-type=fbank"]
        if spec.fbank_config:
            fb: Dict[str, object] = {"num-mel-bins": spec.num_mel_bins, "low-freq": low_freq, "high-freq": high_freq,
                                     "sample-frequency": spec.sample_frequency}
            if spec.dither is not None:
                fb["dither"] = spec.dither
            if spec.frame_length is not None:
                fb["frame-length"] = spec.frame_length
            fb.update(spec.fbank_opts or {})
            (conf / "fbank.conf").write_text("".join(f"--{k}={_conf_value(v)}\n" for k, v in fb.items()))
            online.append(f"--fbank-config={conf / 'fbank.conf'}")
    if spec.ivector_dim > 0:
        ie = model_dir / "model" / "online" / "ivector_extractor"
        write_ivector_extractor(ie, spec)
        (conf / "splice.conf").write_text(f"--left-context={spec.splice_left}\n--right-context={spec.splice_right}\n")
        (conf / "online_cmvn.conf").write_text("# configuration file for apply-cmvn-online, used in the script ../local/run_online_decoding.sh\n")
        ivc = [f"--splice-config={conf / 'splice.conf'}", f"--cmvn-config={conf / 'online_cmvn.conf'}",
               f"--lda-matrix={ie / 'final.mat'}", f"--global-cmvn-stats={ie / 'global_cmvn.stats'}",
               f"--diag-ubm={ie / 'final.dubm'}", f"--ivector-extractor={ie / 'final.ie'}",
               "--num-gselect=5", "--min-post=0.025", "--posterior-scale=0.1",
               "--max-remembered-frames=1000", "--max-count=100", "--ivector-period=10"]
        (conf / "ivector_extractor.conf").write_text("\n".join(ivc) + "\n")
        online.append(f"--ivector-extraction-config={conf / 'ivector_extractor.conf'}")
    if spec.nnet_cmvn:
        if spec.ivector_dim <= 0:
            raise ValueError("nnet_cmvn needs the extractor's global_cmvn.stats")
        (conf / "nnet_cmvn.conf").write_text("--cmn-window=600\n")
        online.append(f"--cmvn-config={conf / 'nnet_cmvn.conf'}")
        online.append(f"--global-cmvn-stats={model_dir / 'model' / 'online' / 'ivector_extractor' / 'global_cmvn.stats'}")
    online.append("--endpoint.silence-phones=1")
    (conf / "online.conf").write_text("\n".join(online) + "\n")


# --------------------------------------------------------------------------- HCLG graphs

_FST_MAGIC = 2125659606


@dataclass
class Fst:
    """Mutable arc list used to assemble a graph before writing it as ConstFst."""
    arcs: List[List[Tuple[int, int, float, int]]] = field(default_factory=list)   # per state: (ilabel, olabel, cost, next)
    finals: Dict[int, float] = field(default_factory=dict)
    start: int = 0

    def add_state(self) -> int:
        self.arcs.append([])
        return len(self.arcs) - 1

    def add_arc(self, s: int, il: int, ol: int, cost: float, n: int) -> None:
        self.arcs[s].append((il, ol, float(np.float32(cost)), n))

    @property
    def num_states(self) -> int:
        return len(self.arcs)

    @property
    def num_arcs(self) -> int:
        return sum(len(a) for a in self.arcs)


def _fst_string(s: str) -> bytes:
    return struct.pack("<i", len(s)) + s.encode()


def write_const_fst(path: Path, fst: Fst) -> None:
    """OpenFst ConstFst<StdArc> v2 (unaligned) binary: header (kaldi/openfst/src/lib/fst.cc:84-96), then
    states {f32 final, u32 pos, u32 narcs, u32 nieps, u32 noeps}, then arcs {i32,i32,f32,i32}
    (include/fst/const-fst.h:102-110).  Arcs are ilabel-sorted per state like mkgraph.sh's output."""
    states = np.zeros(fst.num_states, dtype=[("w", "<f4"), ("pos", "<u4"), ("n", "<u4"), ("ni", "<u4"), ("no", "<u4")])
    arcs = np.zeros(fst.num_arcs, dtype=[("il", "<i4"), ("ol", "<i4"), ("w", "<f4"), ("ns", "<i4")])
    pos = 0
    for s, al in enumerate(fst.arcs):
        al = sorted(al, key=lambda a: (a[0], a[1], a[3]))
        states[s] = (fst.finals.get(s, np.inf), pos, len(al), sum(1 for a in al if a[0] == 0), sum(1 for a in al if a[1] == 0))
        for a in al:
            arcs[pos] = a
            pos += 1
    props = 0x1  # kExpanded; the decoder never looks at the rest
    hdr = struct.pack("<i", _FST_MAGIC) + _fst_string("const") + _fst_string("standard") + struct.pack(
        "<iiQqqq", 2, 0, props, fst.start, fst.num_states, fst.num_arcs)
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(states.tobytes())
        f.write(arcs.tobytes())


def write_vector_fst(path: Path, fst: Fst) -> None:
    """OpenFst VectorFst<StdArc> v2 binary (include/fst/vector-fst.h WriteFst): per state final f32,
    i64 narcs, arcs."""
    hdr = struct.pack("<i", _FST_MAGIC) + _fst_string("vector") + _fst_string("standard") + struct.pack(
        "<iiQqqq", 2, 0, 0x1, fst.start, fst.num_states, fst.num_arcs)
    with open(path, "wb") as f:
        f.write(hdr)
        for s, al in enumerate(fst.arcs):
            al = sorted(al, key=lambda a: (a[0], a[1], a[3]))
            f.write(struct.pack("<fq", fst.finals.get(s, np.inf), len(al)))
            for a in al:
                f.write(struct.pack("<iifi", *a))


DEFAULT_SENTENCES = """
turn on the garage light
turn off the garage light
turn on the living room lamp
turn off the living room lamp
turn on the bedroom light
turn off the bedroom light
what time is it
what is the temperature
how hot is it
how cold is it
is the garage door open
is the garage door closed
set the bedroom light to red
set the bedroom light to green
set the bedroom light to blue
set the living room lamp to red
set the living room lamp to green
set the living room lamp to blue
tell me the time
whats the temperature
open the garage door
close the garage door
set a timer for five minutes
set a timer for ten minutes
set a timer for twenty minutes
stop the timer
pause the music
play the music
next song
previous song
volume up
volume down
turn up the volume
turn down the volume
good morning
good night
""".strip().splitlines()


@dataclass
class Lexicon:
    words: List[str]                      # id = index (0 = <eps>)
    prons: Dict[int, List[int]]           # word id -> phone ids (1-based); phone 1 = silence
    sil_phone: int = 1


def make_lexicon(sentences: Sequence[Sequence[str]], spec: ModelSpec, rng: np.random.Generator,
                 extra_words: int = 0) -> Lexicon:
    vocab = sorted({w for s in sentences for w in s})
    vocab += [f"w{i:05d}" for i in range(extra_words)]
    words = ["<eps>"] + vocab
    prons = {}
    for i in range(1, len(words)):
        n = int(rng.integers(2, 7))
        prons[i] = [int(x) for x in rng.integers(2, spec.num_phones + 1, n)]
    return Lexicon(words, prons)


def _add_phone(fst: Fst, spec: ModelSpec, src: int, phone: int, olabel: int, entry_cost: float, dst: Optional[int] = None) -> int:
    """One HMM instance as add-self-loops leaves it for the 1-emitting-state topologies used here:
    forward arc (forward tid) into a state carrying the self-loop tid (cost -log 0.5 each,
    --self-loop-scale 1.0 / --transition-scale 1.0, kaldi.py:415-425)."""
    sl, fw = transition_ids(spec, phone)
    st = fst.add_state() if dst is None else dst
    fst.add_arc(src, fw, olabel, entry_cost + math.log(2.0), st)
    fst.add_arc(st, sl, 0, math.log(2.0), st)
    return st


def make_grammar_hclg(sentences: Sequence[Sequence[str]], lex: Lexicon, spec: ModelSpec,
                      rng: np.random.Generator) -> Fst:
    """Grammar-style HCLG: prefix tree over the sentences (a determinised G), each word expanded to its
    phone HMMs, optional silence between words through epsilon arcs, sentence-final states."""
    wid = {w: i for i, w in enumerate(lex.words)}
    fst = Fst()
    root = fst.add_state()
    fst.start = root
    # optional leading silence
    g0 = fst.add_state()
    fst.add_arc(root, 0, 0, math.log(2.0), g0)
    s_sil = _add_phone(fst, spec, root, lex.sil_phone, 0, math.log(2.0))
    fst.add_arc(s_sil, 0, 0, 0.0, g0)
    trie: Dict[Tuple[int, ...], int] = {(): g0}
    counts: Dict[Tuple[int, ...], int] = {}
    for s in sentences:
        ids = tuple(wid[w] for w in s)
        for k in range(len(ids) + 1):
            counts[ids[:k]] = counts.get(ids[:k], 0) + 1
    for s in sentences:
        ids = tuple(wid[w] for w in s)
        for k in range(1, len(ids) + 1):
            pre = ids[:k]
            if pre in trie:
                continue
            src = trie[pre[:-1]]
            cost = -math.log(counts[pre] / counts[pre[:-1]])
            cur = src
            for j, ph in enumerate(lex.prons[pre[-1]]):
                cur = _add_phone(fst, spec, cur, ph, pre[-1] if j == 0 else 0, cost if j == 0 else 0.0)
            # word end: optional silence, joined by epsilons at the next grammar state
            nxt = fst.add_state()
            fst.add_arc(cur, 0, 0, math.log(2.0), nxt)
            s_sil = _add_phone(fst, spec, cur, lex.sil_phone, 0, math.log(2.0))
            fst.add_arc(s_sil, 0, 0, 0.0, nxt)
            trie[pre] = nxt
    ends: Dict[Tuple[int, ...], int] = {}
    for s in sentences:
        ids = tuple(wid[w] for w in s)
        ends[ids] = ends.get(ids, 0) + 1
    for ids, c in ends.items():
        fst.finals[trie[ids]] = float(np.float32(-math.log(c / counts[ids])))
    return fst


def make_arpa_hclg(sentences: Sequence[Sequence[str]], lex: Lexicon, spec: ModelSpec,
                   rng: np.random.Generator) -> Fst:
    """ARPA-style HCLG: bigram back-off LM (history states, epsilon back-off arcs to a unigram state that
    fans out to the whole vocabulary) composed with the lexicon.  Exercises epsilon closure and, with a
    large vocabulary, max_active/min_active pruning."""
    wid = {w: i for i, w in enumerate(lex.words)}
    V = len(lex.words) - 1
    uni = np.ones(V + 1)
    uni[0] = 0
    big: Dict[int, Dict[int, int]] = {}
    for s in sentences:
        ids = [wid[w] for w in s]
        prev = 0
        for i in ids:
            uni[i] += 3
            big.setdefault(prev, {})[i] = big.get(prev, {}).get(i, 0) + 1
            prev = i
    uni_p = uni / uni.sum()
    fst = Fst()
    start = fst.add_state()       # sentence start history (<s>)
    fst.start = start
    ug = fst.add_state()          # unigram (back-off) state
    hist: Dict[int, int] = {0: start}

    def hstate(w: int) -> int:
        if w not in hist:
            hist[w] = fst.add_state()
        return hist[w]

    def add_word(src: int, w: int, cost: float, dst: int) -> None:
        cur = src
        pr = lex.prons[w]
        for j, ph in enumerate(pr):
            cur = _add_phone(fst, spec, cur, ph, w if j == 0 else 0, cost if j == 0 else 0.0)
        fst.add_arc(cur, 0, 0, math.log(2.0), dst)
        s_sil = _add_phone(fst, spec, cur, lex.sil_phone, 0, math.log(2.0))
        fst.add_arc(s_sil, 0, 0, 0.0, dst)

    for w in range(1, V + 1):
        add_word(ug, w, -math.log(uni_p[w]), hstate(w))
    for h, nxt in big.items():
        tot = sum(nxt.values())
        lam = tot / (tot + len(nxt))                 # Witten-Bell interpolation weight
        hs = hstate(h)
        for w, c in nxt.items():
            add_word(hs, w, -math.log(lam * c / tot + (1 - lam) * uni_p[w]), hstate(w))
        fst.add_arc(hs, 0, 0, -math.log(1 - lam), ug)
    for w, st in hist.items():
        if w not in big:
            fst.add_arc(st, 0, 0, 0.0, ug)           # unseen history: free back-off
        if w != 0:
            fst.finals[st] = float(np.float32(2.0 if w in big else 1.0))
    fst.finals[ug] = 4.0
    return fst


def write_graph_dir(graph_dir: Path, fst: Fst, lex: Lexicon, const: bool = True) -> None:
    graph_dir = Path(graph_dir)
    graph_dir.mkdir(parents=True, exist_ok=True)
    (write_const_fst if const else write_vector_fst)(graph_dir / "HCLG.fst", fst)
    (graph_dir / "words.txt").write_text("".join(f"{w} {i}\n" for i, w in enumerate(lex.words)))


def make_grammar_graph(graph_dir: Path, spec: ModelSpec, seed: int = 11, sentences: Optional[Sequence[str]] = None) -> Tuple[Fst, Lexicon]:
    rng = np.random.default_rng(seed)
    sents = [s.split() for s in (sentences or DEFAULT_SENTENCES)]
    lex = make_lexicon(sents, spec, rng)
    fst = make_grammar_hclg(sents, lex, spec, rng)
    write_graph_dir(graph_dir, fst, lex)
    return fst, lex


def make_arpa_graph(graph_dir: Path, spec: ModelSpec, seed: int = 13, extra_words: int = 2000,
                    num_random_sentences: int = 3000) -> Tuple[Fst, Lexicon]:
    rng = np.random.default_rng(seed)
    sents = [s.split() for s in DEFAULT_SENTENCES]
    lex = make_lexicon(sents, spec, rng, extra_words=extra_words)
    vocab = lex.words[1:]
    for _ in range(num_random_sentences):
        n = int(rng.integers(2, 8))
        sents.append([vocab[int(i)] for i in rng.integers(0, len(vocab), n)])
    fst = make_arpa_hclg(sents, lex, spec, rng)
    write_graph_dir(graph_dir, fst, lex)
    return fst, lex


# --------------------------------------------------------------------------- audio


def synth_utterance(u: int, num_samples: int = 48000, sample_rate: int = 16000) -> np.ndarray:
    """Deterministic int16 test signal: 5 sinusoids in [100, 4000] Hz with a 4 Hz
    amplitude envelope plus uniform noise, peak ~8000."""
    rng = np.random.default_rng(1000 + u)
    t = np.arange(num_samples, dtype=np.float64) / sample_rate
    x = np.zeros(num_samples)
    for _ in range(5):
        f = rng.uniform(100.0, 4000.0)
        ph = rng.uniform(0, 2 * math.pi)
        fm = rng.uniform(0.5, 3.0)
        x += np.sin(2 * math.pi * f * t + ph + 2.0 * np.sin(2 * math.pi * fm * t))
    env = 0.55 + 0.45 * np.sin(2 * math.pi * 4.0 * t + rng.uniform(0, 2 * math.pi))
    x = x * env * 1500.0 + rng.uniform(-200, 200, num_samples)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def write_wav(path: Path, pcm: np.ndarray, sample_rate: int = 16000) -> None:
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())
