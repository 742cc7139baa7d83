"""Log-mel filterbank (--feature-type=fbank) models: the case table of tests/test_fbank_cpu.py, tests/test_gpu_fbank.py and
tests/gen_fbank_golden.py.  The dictionaries are those of tests/cases.py (tiny specs: 24 phones, 48 pdfs; clips of 1-2 s); what
the reference's two decoder binaries and rs-dump gave for each is in tests/golden/fbank/<case>.npz."""
from pathlib import Path

from tests import cases

GOLDEN = cases.GOLDEN / "fbank"
NBEST = cases.NBEST


def _fb(bins=40, opts=None, **spec):
    s = dict(feature_type="fbank", num_mel_bins=bins)
    if opts:
        s["fbank_opts"] = opts
    s.update(spec)
    return s


_FSF3_LAYERS = cases.CASES["tiny_fsf3_u16"]["spec"]["layer_offsets"]

CASES = {
    # 40 bins, no energy, the iVector extractor on the filterbank rows: the usual recipe
    "fb40_iv": dict(spec=_fb(), graph="grammar", audio="synth:30:32000"),
    # no --fbank-config line at all: the reference's defaults, 23 bins and dither 1.0
    "fb23_default": dict(spec=_fb(23, fbank_config=False, ivector_dim=0), graph="grammar", audio="synth:31:24000"),
    # the last bin count one pass of lanes covers, and the first that needs the second
    "fb64": dict(spec=_fb(64), graph="grammar", audio="synth:32:24000"),
    "fb65": dict(spec=_fb(65), graph="grammar", audio="synth:33:24000"),
    # two bins per lane; 128 columns with the energy.  127 triangles between 20 and 7600 Hz are narrower than a bin of the 512-point
    # FFT at the low end (the reference refuses that: "You may have set --num-mel-bins too large"), so this band starts at 600 Hz
    "fb80_noiv": dict(spec=_fb(80, ivector_dim=0), graph="grammar", audio="synth:34:24000"),
    "fb127_energy": dict(spec=_fb(127, {"use-energy": True, "low-freq": 600, "high-freq": 0}), graph="grammar", audio="synth:35:24000"),
    # the energy in column 0 with the mel columns shifted by one, and in the last column
    "fb40_energy": dict(spec=_fb(40, {"use-energy": True}), graph="grammar", audio="synth:36:24000"),
    "fb40_energy_htk": dict(spec=_fb(40, {"use-energy": True, "htk-compat": True}), graph="grammar", audio="synth:37:24000"),
    # the windowed frame's energy, floored: digital silence without dither, so the floor binds on every frame
    "fb40_winenergy_floor": dict(spec=_fb(40, {"use-energy": True, "raw-energy": False, "energy-floor": 1.0}, dither=0.0),
                                 graph="grammar", audio="zeros:16000"),
    # no log, and the magnitude spectrum without a log, on audio of one or two LSB (the dither is most of it): rows of O(1e3), peaks
    # of 2e4 where the power of a tone falls into one filter.  input_scale stands for the whitening a trained network's first
    # layer would do on rows of that size, so that the log-likelihoods stay where 1e-4 absolute is more than a few ulps; no
    # extractor, whose LDA and UBM the synthetic models scale for rows of O(10)
    "fb40_linear": dict(spec=_fb(40, {"use-log-fbank": False}, ivector_dim=0, input_scale=0.001), graph="grammar", audio="synth:38:24000:0.0002"),
    "fb40_magnitude": dict(spec=_fb(40, {"use-log-fbank": False, "use-power": False}, ivector_dim=0, input_scale=0.01), graph="grammar",
                           audio="synth:39:24000:0.002"),
    # a 1600-sample window: the 2048-point transform
    "fb40_win100": dict(spec=_fb(frame_length=100.0), graph="grammar", audio="synth:40:32000"),
    # the dither of the filterbank's own frame options: off, and a value other than 1
    "fb40_nodither": dict(spec=_fb(dither=0.0), graph="grammar", audio="synth:41:24000"),
    "fb40_dither05": dict(spec=_fb(dither=0.5, ivector_dim=0), graph="grammar", audio="synth:42:24000:0.01"),
    "fb40_nnetcmvn": dict(spec=_fb(nnet_cmvn=True), graph="grammar", audio="synth:43:32000"),
    "fb40_fsf3": dict(spec=_fb(layer_offsets=_FSF3_LAYERS), graph="grammar", audio="synth:44:32000", conf_opts={"frame-subsampling-factor": 3}),
    # 40 phones and an n-gram graph: the token-list search
    "fb40_arpa": dict(spec=_fb(num_phones=40), graph="arpa:60:200", audio="synth:45:32000"),
    # a clip too short for one frame, and exactly one frame (the model of fb40_iv)
    "fb40_len0": dict(spec=_fb(), graph="grammar", audio="synth:46:399"),
    "fb40_len1": dict(spec=_fb(), graph="grammar", audio="synth:46:400"),
}

LINEAR = ("fb40_linear", "fb40_magnitude")      # rows without a log: compared by relative error


def expected_layout(name: str):
    """(dim, bins, energy column or -1) of the case's feature row: feature-fbank.h:93-95, feature-fbank.cc:102,120."""
    s = CASES[name]["spec"]
    o = s.get("fbank_opts", {}) if s.get("fbank_config", True) else {}
    bins = s["num_mel_bins"]
    if not o.get("use-energy", False):
        return bins, bins, -1
    return bins + 1, bins, (bins if o.get("htk-compat", False) else 0)


def model_key(name: str):
    """Cases with the same key decode with one model and one graph."""
    c = CASES[name]
    return repr((sorted(c["spec"].items(), key=str), c["graph"], c.get("conf_opts"), c.get("opts")))


def build_case_files(name: str, root: Path):
    """(model_dir, graph_dir, wav, pcm) of the case under `root`."""
    return cases.build_case_files(CASES[name], root)


def load_golden(name: str):
    import numpy as np
    return np.load(GOLDEN / f"{name}.npz")
