"""Speaker-adaptation cases shared by the tests (tests/test_gpu_stream_adaptation.py, tests/test_stream_adaptation_cpu.py) and the
golden generator (tools/gen_adaptation_golden.py), and the oracle-side restatement of the adaptation state.

A case = a synthetic model of tests/cases.py's kind with --dither=0 (the dither sequence is not continued across utterances), a
few edits of its conf files so that the limits bind on utterances of 2-3 s, and the utterances of ONE speaker in order.  The
reference carries the state from utterance to utterance itself (spk2utt "spk u1 u2 u3"); its outputs live in
tests/golden/adaptation/.

AdaptedOracle restates, on oracle.pipeline's pieces:
  OnlineIvectorFeature::GetAdaptationState   online2/online-ivector-feature.cc:386-396
  OnlineCmvn::GetState                       feat/online-feature.cc:467-487
  LimitFrames                                online2/online-ivector-feature.cc:109-127
  OnlineIvectorEstimationStats::Scale        ivector/ivector-extractor.cc:671-693
  SetAdaptationState / SetCmvnState          online2/online-ivector-feature.cc:445-453
  SmoothOnlineCmvnStats with speaker stats   feat/online-feature.cc:372-419
A state is a dict of float64 arrays laid out like rhasspy_speech_amd._lib.Adaptation.arrays().
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases

GOLDEN_DIR = cases.GOLDEN / "adaptation"
TICK = 1024
F32 = np.float32

# name: spec = ModelSpec arguments (dither=0.0 is added), big, conf = {conf file: {option: value}} appended / replaced in the
# written files, utts = (synth seed, samples) per utterance, endpoint = the --endpoint.* options (utterance 1 stops by them)
ADAPT_CASES: Dict[str, dict] = {}


def _case(name: str, utts, spec=None, big=False, conf=None, endpoint=None) -> None:
    ADAPT_CASES[name] = dict(spec=dict(spec or {}, dither=0.0), big=big, conf=conf or {}, utts=list(utts), endpoint=endpoint)


_case("ad_tiny_3utt", [(101, 40000), (102, 32000), (104, 45000)], conf={"ivector_extractor.conf": {"max-remembered-frames": 150}})
_case("ad_tiny_maxcount0", [(111, 36000), (112, 40000)], conf={"ivector_extractor.conf": {"max-count": 0, "max-remembered-frames": 150}})
_case("ad_tiny_cmvnwin", [(121, 48000), (122, 48000)],
      conf={"online_cmvn.conf": {"cmn-window": 200, "speaker-frames": 100, "global-frames": 50}})
_case("ad_tiny_nnetcmvn", [(131, 40000), (132, 36000)], spec=dict(nnet_cmvn=True), conf={"ivector_extractor.conf": {"max-remembered-frames": 150}})
_case("ad_tiny_fsf3", [(141, 40000), (142, 40000)], conf={"online.conf": {"frame-subsampling-factor": 3}})
# rule5 fires on the utterance length alone: utterance 1 (3 s) passes 2.5 s, the others (2 s) never do
_case("ad_tiny_endpoint", [(151, 48000), (152, 32000), (153, 32000)], conf={"ivector_extractor.conf": {"max-remembered-frames": 150}},
      endpoint={"silence-phones": "1", "rule5.min-utterance-length": 2.5})
_case("ad_zam_2utt", [(161, 40000), (162, 36000)], big=True)


def case_spec(case: dict) -> synth.ModelSpec:
    return synth.ModelSpec(**case["spec"]) if case["big"] else synth.tiny_spec(**case["spec"])


def endpoint_lines(case: dict) -> List[str]:
    return [f"--endpoint.{k}={v}" for k, v in (case["endpoint"] or {}).items()]


def case_audio(case: dict) -> List[np.ndarray]:
    return [synth.synth_utterance(seed, n) for seed, n in case["utts"]]


def build_files(name: str, root: Path):
    """Model + graph + one wav per utterance of a case under `root` -> (model_dir, graph_dir, [wav paths], [pcm])."""
    case = ADAPT_CASES[name]
    base = dict(spec=case["spec"], big=case["big"], graph="grammar", audio="zeros:0")
    model_dir, graph_dir, _, _ = cases.build_case_files(base, root)
    conf_dir = model_dir / "model" / "online" / "conf"
    for fname, edits in case["conf"].items():
        path = conf_dir / fname
        keep = [l for l in path.read_text().splitlines() if not any(l.startswith(f"--{k}=") for k in edits)]
        path.write_text("\n".join(keep + [f"--{k}={v}" for k, v in edits.items()]) + "\n")
    if case["endpoint"]:
        conf = conf_dir / "online.conf"
        conf.write_text(conf.read_text() + "".join(l + "\n" for l in endpoint_lines(case)))
    pcms = case_audio(case)
    wavs = []
    for i, pcm in enumerate(pcms):
        wavs.append(root / f"u{i + 1}.wav")
        synth.write_wav(wavs[-1], pcm)
    return model_dir, graph_dir, wavs, pcms


def last_read_completes_a_chunk(orc, n_samples: int) -> bool:
    """online2-wav-nnet3-latgen-faster calls InputFinished() BEFORE the AdvanceDecoding of its last chunk (:262-268), the stream
    binary after the one of its last read (online2-cli-nnet3-decode-faster.cc:143-170): a nnet chunk that the last read completes
    gets its iVector from every frame there and from the frames of that read here.  The goldens come from the former and the
    streams restate the latter, so a case's utterances keep clear of it."""
    _, R = orc.nnet.context()
    last = (n_samples - 1) // TICK * TICK      # samples before the last read
    ready = lambda n: max(0, orc.mfcc.num_frames(n) - R) // orc.chunk
    return ready(n_samples) != ready(last)


def load_golden(name: str) -> dict:
    return json.loads((GOLDEN_DIR / f"{name}.json").read_text())


# ------------------------------------------------------------------------------------------------ packed symmetric matrices
def pack(m: np.ndarray) -> np.ndarray:
    """Lower triangle row by row (SpMatrix)."""
    return np.asarray(m, np.float64)[np.tril_indices(m.shape[0])].copy()


def unpack(p: np.ndarray, dim: int) -> np.ndarray:
    m = np.zeros((dim, dim))
    m[np.tril_indices(dim)] = p
    return m + np.tril(m, -1).T


def diag_index(dim: int) -> np.ndarray:
    r = np.arange(dim)
    return r * (r + 1) // 2 + r


# ------------------------------------------------------------------------------------------------ the state's arithmetic
def scale_stats(lin: np.ndarray, quad_packed: np.ndarray, num_frames: float, scale: float, prior_offset: float, max_count: float):
    """OnlineIvectorEstimationStats::Scale (ivector-extractor.cc:671-693) on a packed quadratic term -> (lin, quad, num_frames)."""
    assert 0.0 <= scale <= 1.0
    old = num_frames
    num_frames = num_frames * scale
    quad = quad_packed * scale
    lin = lin * scale
    d = diag_index(len(lin))
    if max_count == 0.0:
        lin[0] += prior_offset * (1.0 - scale)
        quad[d] += 1.0 - scale
    else:
        old_prior_scale = scale * max(old, max_count) / max_count
        new_prior_scale = max(num_frames, max_count) / max_count
        lin[0] += prior_offset * (new_prior_scale - old_prior_scale)
        quad[d] += new_prior_scale - old_prior_scale
    return lin, quad, num_frames


def limit_frames(state: dict, max_remembered_frames: float, posterior_scale: float, prior_offset: float, max_count: float) -> dict:
    """LimitFrames (online-ivector-feature.cc:109-127), BaseFloat where the reference has BaseFloat.  The nnet-input block is not
    touched."""
    out = {k: np.array(v, np.float64) for k, v in state.items()}
    mrf = F32(max_remembered_frames)
    if out["cmvn_ivector"].size:
        C1 = out["cmvn_ivector"].size // 2
        count = F32(out["cmvn_ivector"][C1 - 1])
        if count > mrf:
            out["cmvn_ivector"] = out["cmvn_ivector"] * float(F32(mrf / count))
    if out["ivector_count"].size:
        target = F32(mrf * F32(posterior_scale))
        nf = float(out["ivector_count"][0])
        if nf > float(target):
            lin, quad, nf = scale_stats(out["ivector_linear"], out["ivector_quadratic"], nf, float(target) / nf, prior_offset, max_count)
            out["ivector_linear"], out["ivector_quadratic"], out["ivector_count"] = lin, quad, np.array([nf])
    return out


def online_cmvn_speaker(feats: np.ndarray, global_stats: np.ndarray, speaker_stats: Optional[np.ndarray], cmn_window: int = 600,
                        speaker_frames: int = 600, global_frames: int = 200) -> np.ndarray:
    """pipeline.online_cmvn with SmoothOnlineCmvnStats' speaker term: speaker_stats = 2 x (C + 1) flattened, or None / count 0."""
    T, C = feats.shape
    x = feats.astype(np.float64)
    cs = np.concatenate([np.zeros((1, C)), np.cumsum(x, 0)])
    t = np.arange(T)
    lo = np.maximum(0, t + 1 - cmn_window)
    s = cs[t + 1] - cs[lo]
    n = (t + 1 - lo).astype(np.float64)
    if speaker_stats is not None and len(speaker_stats) and speaker_stats[C] > 0.0:
        scount = float(speaker_stats[C])
        from_speaker = np.minimum(np.minimum(np.maximum(cmn_window - n, 0.0), float(speaker_frames)), scount)
        b = from_speaker / scount
        s = s + b[:, None] * np.asarray(speaker_stats[:C], np.float64)[None, :]
        n = n + b * scount
    from_global = np.minimum(np.maximum(cmn_window - n, 0.0), float(global_frames))
    gcount = global_stats[0, C]
    a = from_global / gcount
    s = s + a[:, None] * global_stats[0, :C][None, :]
    n = n + a * gcount
    alpha = (-1.0 / n).astype(F32).astype(np.float64)
    offset = (alpha[:, None] * s).astype(F32)
    return (feats + offset).astype(F32)


def accumulate_cmvn(block: np.ndarray, feats: np.ndarray) -> np.ndarray:
    """OnlineCmvn::GetState: block (2 x (C + 1), flattened) + (1, x, x^2) per frame, in frame order, in double."""
    T, C = feats.shape
    out = np.array(block, np.float64) if len(block) else np.zeros(2 * (C + 1))
    x = feats.astype(np.float64)
    for t in range(T):
        out[C] += 1.0
        out[:C] += x[t]
        out[C + 1:2 * C + 1] += x[t] * x[t]
    return out


class AdaptedOracle:
    """The stream oracle of oracle.pipeline with an adaptation state going in and coming out."""

    def __init__(self, orc, model_dir):
        from oracle import kaldi_formats as kf
        self.orc = orc
        conf_dir = Path(model_dir) / "model" / "online" / "conf"
        online = dict(kf.read_config(conf_dir / "online.conf"))

        def cmvn_opts(path):
            c = dict(kf.read_config(path))
            return dict(cmn_window=int(c.get("cmn-window", 600)), speaker_frames=int(c.get("speaker-frames", 600)), global_frames=int(c.get("global-frames", 200)))

        self.iv_cmvn = self.nn_cmvn = None
        self.max_remembered_frames = 1000.0
        if orc.ie is not None:
            ic = dict(kf.read_config(online["ivector-extraction-config"]))
            self.iv_cmvn = cmvn_opts(ic["cmvn-config"])
            self.max_remembered_frames = float(ic.get("max-remembered-frames", 1000))
        if orc.nnet_cmvn is not None:
            self.nn_cmvn = cmvn_opts(online["cmvn-config"])

    def fresh(self) -> dict:
        from oracle import pipeline
        orc, e = self.orc, np.zeros(0)
        C = orc.mfcc.o.num_ceps
        st = dict(ivector_linear=e, ivector_quadratic=e, ivector_count=e, cmvn_ivector=e, cmvn_nnet=e)
        if orc.ie is not None:
            s = pipeline.IvectorStats(orc.ie["ext"], orc.ie["max_count"])
            st.update(ivector_linear=s.lin.copy(), ivector_quadratic=pack(s.quad), ivector_count=np.zeros(1), cmvn_ivector=np.zeros(2 * (C + 1)))
        if orc.nnet_cmvn is not None:
            st["cmvn_nnet"] = np.zeros(2 * (C + 1))
        return st

    def run(self, pcm: np.ndarray, state: dict, stop_tick: Optional[int] = None, nbest: int = 1):
        """One utterance opened with `state`; stop_tick: finalize after that many + 1 complete ticks (no flush), else finish.
        -> (pipeline.Transcript, the state after it)."""
        from oracle import lattice as lat
        from oracle import pipeline
        orc = self.orc
        pcm = np.asarray(pcm)
        n_used = len(pcm) if stop_tick is None else TICK * (stop_tick + 1)
        feats = orc.features(pcm[:n_used])
        T = feats.shape[0]
        sched, L, R = orc.stream_schedule(n_used)
        if stop_tick is not None:
            sched = [c for c in sched if c[0] <= stop_tick]      # nothing is flushed
        nn_in = feats if orc.nnet_cmvn is None else online_cmvn_speaker(feats, orc.nnet_cmvn, state["cmvn_nnet"], **self.nn_cmvn)
        ivs, st = None, None
        if orc.ie is not None:
            ie = orc.ie
            I = ie["ext"].M.shape[2]
            cm = online_cmvn_speaker(feats, ie["gstats"], state["cmvn_ivector"], **self.iv_cmvn)
            st = pipeline.IvectorStats(ie["ext"], ie["max_count"])
            st.lin, st.quad, st.num_frames = np.array(state["ivector_linear"], np.float64), unpack(state["ivector_quadratic"], I), float(state["ivector_count"][0])
            x = np.zeros(I)
            x[0] = ie["ext"].prior_offset
            done, rows = 0, []
            for (_, last) in sched:
                if last + 1 > done:
                    T_ready = T if last == T - 1 else last + 1 + ie["right"]
                    orc._ivector_acc(st, feats, cm, done, last + 1, min(T_ready, T))
                    done = last + 1
                    x = st.get_ivector(x)
                out = x.astype(F32)
                out[0] = F32(np.float64(out[0]) - ie["ext"].prior_offset)
                rows.append(out)
            ivs = np.stack(rows)
            H = orc.nnet.halo
            ts = np.arange(-H, T + H)
            slot = (ts // orc.chunk) * orc.chunk
            provider = {}
            ends = [orc.chunk * (k + 1) + R for k in range(len(sched))]
            for k in range(len(sched)):
                for t in range(-L if k == 0 else ends[k - 1], ends[k]):
                    provider.setdefault((t // orc.chunk) * orc.chunk, k)
            maxk = len(sched) - 1
            idx = np.array([min(provider.get(int(sl), maxk if sl > 0 else 0), maxk) for sl in slot])
            ll = orc.nnet.forward(nn_in, ivs[idx], orc.acoustic_scale)
        else:
            ll = orc.nnet.forward(nn_in, None, orc.acoustic_scale)
        t1 = T if stop_tick is None else min(orc.chunk * len(sched), T)
        ll = np.ascontiguousarray(ll[:t1][::orc.fsf])
        lattice, ctr = pipeline.decode(orc.fst, orc.id2pdf, ll, **orc.opts)
        paths = lat.nbest(lattice, nbest, orc.opts["lattice_beam"], 1.0)
        tr = pipeline.Transcript(ll.shape[0], nn_in, ivs, ll, paths, lattice, ctr)
        # ---- GetAdaptationState / GetCmvnState
        new = {k: np.array(v, np.float64) for k, v in state.items()}
        if orc.ie is not None:
            new["cmvn_ivector"] = accumulate_cmvn(state["cmvn_ivector"], feats)
            new["ivector_linear"], new["ivector_quadratic"], new["ivector_count"] = st.lin.copy(), pack(st.quad), np.array([st.num_frames])
            new = limit_frames(new, self.max_remembered_frames, orc.ie["posterior_scale"], orc.ie["ext"].prior_offset, orc.ie["max_count"])
        if orc.nnet_cmvn is not None:
            new["cmvn_nnet"] = accumulate_cmvn(state["cmvn_nnet"], feats)
        return tr, new
