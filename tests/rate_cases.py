"""Models of sampling rates other than 16 kHz: the case table of tests/test_rates_cpu.py, tests/test_gpu_rates.py and
tests/gen_rate_golden.py.  Tiny specs as in tests/fbank_cases.py (24 phones, 48 pdfs), clips of at most 1.5 s at the case's own rate;
what the reference's two decoder binaries and rs-dump gave for each is in tests/golden/rates/<case>.npz.

The rate decides the window (25 ms: 200 samples at 8 kHz, 551 at 22.05 kHz, 1200 at 48 kHz), the window decides the transform it is
padded to -- 256, 512, 1024 or 2048 points -- and with it the feature kernel's instantiation.  The mel band of every case is one the
reference accepts at that rate and transform ("You may have set --num-mel-bins too large" otherwise): 40 Hz to 200 Hz below Nyquist
for the 8 kHz models as in Kaldi's own mfcc_hires for 8 kHz, 20 Hz to 400 Hz below Nyquist for the others as at 16 kHz."""
from pathlib import Path

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases

GOLDEN = cases.GOLDEN / "rates"
NBEST = cases.NBEST

_FSF3_LAYERS = cases.CASES["tiny_fsf3_u16"]["spec"]["layer_offsets"]


def _r8k(**spec):
    s = dict(sample_frequency=8000, low_freq=40, high_freq=-200)
    s.update(spec)
    return s


CASES = {
    # name: spec, graph, audio = synth:<seed>:<samples> at the spec's rate
    # hires MFCC (40 bins, 40 cepstra) with the iVector extractor: the usual telephone recipe.  200 samples -> 256 points
    "r8k_iv": dict(spec=_r8k(), graph="grammar", audio="synth:80:11000"),
    # mfcc.conf with the rate and --use-energy=false only: the reference's defaults (23 bins from 20 Hz to Nyquist, 13 cepstra, dither 1.0)
    "r8k_default": dict(spec=dict(sample_frequency=8000, mfcc_defaults=True, num_mel_bins=23, num_ceps=13, ivector_dim=0), graph="grammar",
                        audio="synth:81:10000"),
    # log-mel filterbank rows with the energy in column 0: FbankKernel<256>
    "r8k_fbank40": dict(spec=_r8k(feature_type="fbank", fbank_opts={"use-energy": True}), graph="grammar", audio="synth:82:10000"),
    # the chunk schedule of a subsampled network at a shift of 80 samples
    "r8k_fsf3": dict(spec=_r8k(layer_offsets=_FSF3_LAYERS), graph="grammar", audio="synth:83:12000", conf_opts={"frame-subsampling-factor": 3}),
    # the window as long as the transform (no zero tail), shorter than usual (the clamped pair loads reach far into the wave), and one
    # that no longer fits 256 points: the 512-point kernel at another rate
    "r8k_win32": dict(spec=_r8k(frame_length=32.0), graph="grammar", audio="synth:84:10000"),
    "r8k_win20": dict(spec=_r8k(frame_length=20.0), graph="grammar", audio="synth:85:10000"),
    "r8k_win33": dict(spec=_r8k(frame_length=33.0), graph="grammar", audio="synth:86:10000"),
    # 40 phones and an n-gram graph: the token-list search behind the 256-point front end
    "r8k_arpa": dict(spec=_r8k(num_phones=40), graph="arpa:60:200", audio="synth:87:12000"),
    # one sample short of a frame, and exactly one frame (the model of r8k_iv)
    "r8k_len0": dict(spec=_r8k(), graph="grammar", audio="synth:88:199"),
    "r8k_len1": dict(spec=_r8k(), graph="grammar", audio="synth:88:200"),
    # 275 samples, odd: the unpaired loads of the 512-point kernel
    "r11k": dict(spec=dict(sample_frequency=11025), graph="grammar", audio="synth:89:15000"),
    # 551 samples, odd -> 1024 points
    "r22k": dict(spec=dict(sample_frequency=22050), graph="grammar", audio="synth:90:30000"),
    # 800 samples -> 1024 points, 80 filterbank bins: FbankKernel<1024> with its second pass of mel lanes
    "r32k_fbank": dict(spec=dict(sample_frequency=32000, feature_type="fbank", num_mel_bins=80), graph="grammar", audio="synth:91:44000"),
    # 1102 samples -> 2048 points at an odd shift of 441: every second frame starts on a 2-byte boundary only
    "r44k": dict(spec=dict(sample_frequency=44100), graph="grammar", audio="synth:92:60000"),
    # 1200 samples -> 2048 points
    "r48k": dict(spec=dict(sample_frequency=48000), graph="grammar", audio="synth:93:66000"),
}

NO_FRAME = "r8k_len0"
DECODED = [n for n in CASES if n != NO_FRAME]


def rate(name: str) -> int:
    return CASES[name]["spec"]["sample_frequency"]


def geometry(name: str):
    """(window, shift, padded window) in samples: feature-window.h:73-86 in the float arithmetic of model.h."""
    s = CASES[name]["spec"]
    f = np.float32(rate(name)) * np.float32(0.001)
    win, shift = int(f * np.float32(s.get("frame_length", 25.0))), int(f * np.float32(10.0))
    return win, shift, 1 << (win - 1).bit_length()


def feat_dim(name: str) -> int:
    return synth.tiny_spec(**CASES[name]["spec"]).feat_dim


def num_frames(name: str, n_samples: int) -> int:
    win, shift, _ = geometry(name)
    return 0 if n_samples < win else 1 + (n_samples - win) // shift


def model_key(name: str):
    """Cases with the same key decode with one model and one graph."""
    c = CASES[name]
    return repr((sorted(c["spec"].items(), key=str), c["graph"], c.get("conf_opts"), c.get("opts")))


def case_audio(name: str) -> np.ndarray:
    kind, seed, n = CASES[name]["audio"].split(":")
    assert kind == "synth"
    pcm = synth.synth_utterance(int(seed), int(n), rate(name))
    assert len(pcm) <= 1.5 * rate(name)
    return pcm


def build_case_files(name: str, root: Path):
    """(model_dir, graph_dir, wav, pcm) of the case under `root`: the model and graph as tests/cases.py writes them, the clip and
    its wav at the case's rate."""
    model_dir, graph_dir, wav, _ = cases.build_case_files(dict(CASES[name], audio="zeros:0"), root)
    pcm = case_audio(name)
    synth.write_wav(wav, pcm, rate(name))
    return model_dir, graph_dir, wav, pcm


def load_golden(name: str):
    return np.load(GOLDEN / f"{name}.npz")


# ---- the CPU restatement (oracle/pipeline.py) of a case.  Its front end is written for MFCC rows; for the two filterbank cases the
# rows come from the same pieces -- its window, dither table, frame sum, FFT and mel matrix -- put together as feature-fbank.cc:72-123
# does, and everything behind the rows is the oracle's own.
class _FbankFront:
    def __init__(self, mfcc, use_energy: bool):
        self.m, self.use_energy = mfcc, use_energy
        self.o, self.win, self.shift, self.padded, self.rand_offset = mfcc.o, mfcc.win, mfcc.shift, mfcc.padded, mfcc.rand_offset

    def num_frames(self, n: int) -> int:
        return self.m.num_frames(n)

    def compute(self, pcm: np.ndarray) -> np.ndarray:
        from oracle import pipeline as pl
        F32, m = np.float32, self.m
        T = m.num_frames(len(pcm))
        dim = m.o.num_bins + (1 if self.use_energy else 0)
        if T == 0:
            return np.zeros((0, dim), F32)
        fr = pcm.astype(F32)[np.arange(T)[:, None] * m.shift + np.arange(m.win)[None, :]]
        if m.o.dither != 0.0:
            fr = fr + pl.dither_table(T, m.win, m.rand_offset) * F32(m.o.dither)
        fr = fr - (pl.frame_sum(fr) / F32(m.win))[:, None]
        energy = np.log(np.maximum((fr.astype(np.float64) ** 2).sum(1), np.finfo(F32).eps)).astype(F32)      # raw energy: before pre-emphasis
        pre = fr.copy()
        pre[:, 1:] = fr[:, 1:] - F32(m.o.preemph) * fr[:, :-1]
        pre[:, 0] = fr[:, 0] - F32(m.o.preemph) * fr[:, 0]
        pre *= m.window[None, :]
        pad = np.zeros((T, m.padded), F32)
        pad[:, :m.win] = pre
        mel = np.log(np.maximum(m.fft.power_spectrum(pad) @ m.melW.T, np.finfo(F32).eps)).astype(F32)
        return np.concatenate([energy[:, None], mel], axis=1) if self.use_energy else mel


def make_oracle(name: str, model_dir: Path, graph_dir: Path, scratch: Path):
    """oracle.pipeline.Oracle on the case's files."""
    from oracle import kaldi_formats as kf
    from oracle import pipeline as pl
    spec = CASES[name]["spec"]
    if spec.get("feature_type", "mfcc") == "mfcc":
        return pl.Oracle(model_dir, graph_dir)
    # a copy of the configuration that names the filterbank's frame and mel options as an MFCC's, for the oracle to read
    conf = model_dir / "model" / "online" / "conf"
    fb = dict(kf.read_config(conf / "fbank.conf"))
    use_energy = fb.pop("use-energy", "false") == "true"
    alias = scratch / "model" / "online" / "conf"
    alias.mkdir(parents=True)
    (scratch / "model" / "model").mkdir()
    (scratch / "model" / "model" / "final.mdl").symlink_to(model_dir / "model" / "model" / "final.mdl")
    (alias / "mfcc.conf").write_text("".join(f"--{k}={v}\n" for k, v in fb.items()) + f"--num-ceps={fb['num-mel-bins']}\n--use-energy=false\n")
    lines = [ln for ln in (conf / "online.conf").read_text().splitlines() if not ln.startswith(("--feature-type", "--fbank-config"))]
    (alias / "online.conf").write_text("\n".join(["--feature-type=mfcc", f"--mfcc-config={alias / 'mfcc.conf'}"] + lines) + "\n")
    orc = pl.Oracle(scratch, graph_dir)
    orc.mfcc = _FbankFront(orc.mfcc, use_energy)
    return orc
