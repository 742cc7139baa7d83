"""Utterance-length edge cases (tests/test_length_edges_cpu.py, tests/test_gpu_length_edges.py, oracle/gen_length_golden.py): eight
model variants, each decoded at the lengths where length-dependent code changes its path -- one frame up, the streaming chunk and
1024-sample tick edges, clips too short for a frame, the online CMVN's 200- and 600-frame edges.  The audio of every case is a
prefix of ONE utterance per variant, so shorter cases nest inside longer ones.  Deterministic: the same table here and in the
build container where the reference produced tests/golden/lengths/<variant>.npz."""
from pathlib import Path

import numpy as np

from tests import cases

GOLDEN = cases.GOLDEN / "lengths"
FULL = 97000          # samples of a variant's utterance: 604 frames of 25 ms
SHIFT = 160
TICK = 1024           # what online2-cli-nnet3-decode-faster reads at a time

# spec / graph / opts / conf_opts: the dictionaries of tests/cases.py; seed: the utterance (synth.synth_utterance(seed, FULL));
# classes: the length classes below
VARIANTS = {
    "V1": dict(spec=dict(), graph="grammar", seed=101, classes="ABCDE"),
    "V2": dict(spec=dict(ivector_dim=0), graph="grammar", seed=102, classes="ABCD"),
    "V3": dict(spec=dict(nnet_cmvn=True), graph="grammar", seed=103, classes="ABCDE"),
    # L = R = 6, the decoder sees every third frame
    "V4": dict(spec=dict(cases.CASES["tiny_fsf3_u16"]["spec"]), graph="grammar", seed=104, classes="ABCD",
               conf_opts={"frame-subsampling-factor": 3}),
    # TdnnComponent bottlenecks, priors, log-softmax
    "V5": dict(spec=dict(cases.CASES["tinyf_u5"]["spec"]), graph="grammar", seed=105, classes="ABCD"),
    # min-active binds from the first frame
    "V6": dict(spec=dict(num_phones=40), graph="arpa:300:1500", seed=106, classes="ABCD", opts=dict(max_active=60, min_active=20, beam=12.0)),
    # a 1600-sample window: 400 and 1599 samples give no frame
    "V7": dict(spec=dict(frame_length=100.0), graph="grammar", seed=107, classes="ABCD"),
    # the zamia-size model: the wide-layer split-fp16 GEMM, 128/160-row tiles
    # (classes "8": not a class of its own but V8's short list -- V8_FRAMES, filed under A / B, and 399 samples under D)
    "V8": dict(big=True, spec=dict(), graph="grammar", seed=108, classes="8"),
}

CLASS_A = [(T, 0) for T in range(1, 13)] + [(1, 159), (2, 0)]                  # frame edges: (T, extra samples)
CLASS_B = [23, 24, 25, 27, 28, 29, 30, 31, 47, 48, 49]                         # chunk edges for chunk 24, R = 4 or 6 (frames)
CLASS_C = [1023, 1024, 1025, 2047, 2048, 2049, 4719, 4720, 5119, 5120, 5121]   # tick edges (samples)
CLASS_E = [199, 200, 201, 599, 600, 601, 602]                                  # online CMVN: global-stats blend, sliding window (frames)
V8_FRAMES = [1, 2, 3, 5, 8, 12, 24, 25, 29]


def window(variant: str) -> int:
    """Samples of the first frame: 400, or 1600 with --frame-length=100."""
    fl = VARIANTS[variant]["spec"].get("frame_length")
    return 400 if fl is None else int(round(16.0 * fl))


def samples(variant: str, T: int, extra: int = 0) -> int:
    """n(T, j) = w + 160 (T - 1) + j: the shortest clip of T frames, plus j samples."""
    return window(variant) + SHIFT * (T - 1) + extra


def num_frames(variant: str, n: int) -> int:
    w = window(variant)
    return 0 if n < w else 1 + (n - w) // SHIFT


def lengths(variant: str) -> dict:
    """{n: classes that ask for n}, by ascending n."""
    w = window(variant)
    out = {}

    def add(n, cls):
        out[n] = out.get(n, "") + cls
    for cls in VARIANTS[variant]["classes"]:
        if cls == "A":
            for T, j in CLASS_A:
                add(samples(variant, T, j), "A")
        elif cls == "B":
            for T in CLASS_B:
                add(samples(variant, T), "B")
        elif cls == "C":
            for n in CLASS_C:
                add(n, "C")
        elif cls == "D":
            for n in sorted({0, 1, w - 1} | ({400} if w > 400 else set())):
                add(n, "D")
        elif cls == "E":
            for T in CLASS_E:
                add(samples(variant, T), "E")
        elif cls == "8":      # V8 only: a few frame and chunk edges and one clip without a frame
            for T in V8_FRAMES:
                add(samples(variant, T), "A" if T <= 12 else "B")
            add(399, "D")
    return dict(sorted(out.items()))


def case(variant: str) -> dict:
    """The variant as a case dictionary of tests/cases.py (audio: the whole utterance)."""
    v = VARIANTS[variant]
    c = {k: v[k] for k in ("spec", "graph", "opts", "conf_opts", "big") if k in v}
    c["audio"] = f"synth:{v['seed']}:{FULL}"
    return c


def build_variant_files(variant: str, root: Path):
    """Model and graph of the variant under `root`; returns (model_dir, graph_dir, pcm of the whole utterance)."""
    model_dir, graph_dir, _wav, pcm = cases.build_case_files(case(variant), root)
    return model_dir, graph_dir, pcm


def key(n: int) -> str:
    """Prefix of a case's arrays in the variant's golden file."""
    return f"n{n}"


def load_golden(variant: str) -> dict:
    """The variant's golden file (and <variant>_stream.npz where the streamed runs have their own) as a dictionary, with the features
    that are stored once (n<n>_input_of = (m, rows): the first rows of the clip of m samples, oracle/gen_length_golden.py) put back
    under n<n>_input."""
    g = {}
    for path in (GOLDEN / f"{variant}.npz", GOLDEN / f"{variant}_stream.npz"):
        if path.exists():
            with np.load(path) as z:
                g.update({k: z[k] for k in z.files})
    for k in [k for k in g if k.endswith("_input_of")]:
        m, rows = (int(x) for x in g[k])
        g[k[:-3]] = g[f"{key(m)}_input"][:rows]
    return g


def stored_rows(g, n: int, mode: str, T: int) -> np.ndarray:
    """Row indices of the case's stored log-likelihoods (all of them unless the file keeps a sample: class E)."""
    k = f"{key(n)}_{mode}_loglike_rows"
    return g[k] if k in g else np.arange(T)


NO_FRAMES = "You cannot get a lattice if you decoded no frames."      # online-nnet3-decoding.cc:69


def reference_error(g, n: int, mode: str) -> str:
    """What a failed reference run said, as far as an interface that takes samples can say it too: the GetLattice error of a clip
    without a frame.  The one other failure in the table is the offline binary on NO samples: its wav reader rejects the file
    ("WaveData: empty file (no data)", wave-reader.cc:301; the recorded end of stderr is the table reader's "Error reading object
    from stream .../utt.wav") before the pipeline sees anything.  The oracle and the library are handed samples, not a file: the
    same clip through online2-cli-nnet3-decode-faster, which reads samples, fails in GetLattice, and that is what they must say."""
    err = bytes(g[f"{key(n)}_{mode}_stderr"]).decode(errors="replace")
    if NO_FRAMES in err:
        return NO_FRAMES
    assert n == 0 and mode == "offline" and "Error reading object from stream" in err and "utt.wav" in err, (n, mode, err)
    assert NO_FRAMES in bytes(g[f"{key(n)}_stream_stderr"]).decode(errors="replace")
    return NO_FRAMES
