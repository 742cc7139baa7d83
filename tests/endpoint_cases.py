"""Endpoint-detection cases shared by the GPU tests (tests/test_gpu_stream_endpoint.py) and the golden generator
(tools/gen_endpoint_golden.py), and the oracle-side restatement of the two quantities the rules are evaluated on.

A case = a parity case of tests/cases.py (model + graph), its audio with a stretch appended, and the --endpoint.* lines appended to
online.conf.  The synthetic acoustic models are random, so "silence" is whatever the case's --endpoint.silence-phones says: the
lists and thresholds below were chosen (tools/gen_endpoint_golden.py --explore prints what the oracle sees on every tick) so that the
rules fire on a known tick, well clear of their thresholds.  Expected outputs of the reference live in tests/golden/endpoint/.
"""
from __future__ import annotations

import copy
import json
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from rhasspy_speech_amd import synth
from tests import cases

GOLDEN_DIR = cases.GOLDEN / "endpoint"
TICK = 1024

# name: base = the case of tests/cases.py; tail = "kind:samples[:scale]" appended to its audio (synth: another synthetic utterance,
# quiet: one scaled down to a few LSB, zeros); lines = the --endpoint.* options (without the leading --endpoint.)
ENDPOINT_CASES: Dict[str, dict] = {}


def _case(name: str, base: str, tail: Optional[str], lines: dict) -> None:
    ENDPOINT_CASES[name] = dict(base=base, tail=tail, lines=lines)


# The random models sit in one phone for most of an utterance, so the "silence" lists below name the phones of that stretch.
# -- cases on which the reference stops before its last chunk
_case("ep_tiny_u0_rule2", "tiny_u0", None, {"silence-phones": "10:19"})                      # rule2's max-relative-cost 2.0 decides the tick
_case("ep_tiny_noiv_rule3", "tiny_noiv_u2", None, {"silence-phones": "9", "rule3.max-relative-cost": 9.7})
_case("ep_tiny_hmm_rule1", "tiny_hmm_u6", None, {"silence-phones": "11", "rule1.min-trailing-silence": 1.3})      # all silence
_case("ep_tiny_cmvn_rule4", "tiny_cmvn_u4", None, {"silence-phones": "10", "rule3.min-trailing-silence": 9.0, "rule4.min-trailing-silence": 1.5})
_case("ep_tiny_fsf3_rule5", "tiny_fsf3_u16", None, {"silence-phones": "1", "rule5.min-utterance-length": 1.6})
_case("ep_zam_u0_rule3", "zam_u0", None, {"silence-phones": "593", "rule3.max-relative-cost": 29.0})
_case("ep_zam_u1_rule2", "zam_u1", None, {"silence-phones": "656", "rule2.max-relative-cost": 28.1})
_case("ep_zam_fsf3_rule1", "zam_fsf3_u19", None, {"silence-phones": "656:728", "rule1.min-trailing-silence": 1.1, "rule2.min-trailing-silence": 0.6})
_case("ep_tinyf_tail_rule5", "tinyf_u5", "synth:32000:41", {"silence-phones": "1", "rule5.min-utterance-length": 3.3})
_case("ep_tiny_arpa_rule1", "tiny_arpa_u7", None, {"silence-phones": "29", "rule1.min-trailing-silence": 2.2, "rule1.max-relative-cost": 5.0})
# -- cases on which it never stops
_case("ep_tiny_text_never", "tiny_text_u1", "quiet:16000:42:0.002", {"silence-phones": "8:10"})
_case("ep_tiny_u0_never", "tiny_u0", None, {"silence-phones": "10:19", "rule2.max-relative-cost": 1.0, "rule3.max-relative-cost": 1.5,
                                            "rule4.min-trailing-silence": 4.0})



def endpoint_lines(case: dict) -> List[str]:
    return [f"--endpoint.{k}={v}" for k, v in case["lines"].items()]


def case_audio(case: dict) -> np.ndarray:
    pcm = cases.case_audio(cases.CASES[case["base"]])
    if case.get("tail"):
        kind, *rest = case["tail"].split(":")
        n = int(rest[0])
        if kind == "zeros":
            extra = np.zeros(n, np.int16)
        else:
            extra = synth.synth_utterance(int(rest[1]), n)
            if len(rest) > 2:
                extra = np.round(extra.astype(np.float64) * float(rest[2])).astype(np.int16)
        pcm = np.concatenate([pcm, extra])
    return pcm


def build_files(name: str, root: Path):
    """Model + graph + wav of an endpoint case under `root` -> (model_dir, graph_dir, wav_path, pcm)."""
    case = ENDPOINT_CASES[name]
    model_dir, graph_dir, _, _ = cases.build_case_files(cases.CASES[case["base"]], root)
    conf = model_dir / "model" / "online" / "conf" / "online.conf"
    conf.write_text(conf.read_text() + "".join(l + "\n" for l in endpoint_lines(case)))
    pcm = case_audio(case)
    wav = root / "utt_endpoint.wav"
    synth.write_wav(wav, pcm)
    return model_dir, graph_dir, wav, pcm


def load_golden(name: str) -> dict:
    return json.loads((GOLDEN_DIR / f"{name}.json").read_text())


def tid_to_phone(spec: synth.ModelSpec) -> np.ndarray:
    """TransitionIdToPhone of the synthetic models: two transition-ids per tuple, in tuple order (synth.tid_to_pdf)."""
    tuples = synth.context_tuples(spec)
    out = np.zeros(2 * len(tuples) + 1, dtype=np.int32)
    for k, (p, _hs, _fwd, _slf) in enumerate(tuples):
        out[2 * k + 1] = out[2 * k + 2] = p
    return out


def frame_shift(orc) -> float:
    """Feature frame shift in seconds x frame-subsampling-factor, in float like the reference (online-nnet3-decoding.cc:90-92)."""
    return float(np.float32(orc.mfcc.o.frame_shift_ms) / np.float32(1000.0) * np.float32(orc.fsf))


def frames_after_ticks(orc, n_samples: int) -> List[int]:
    """Decoder frames searched once the first j + 1 ticks of 1024 samples are complete, j = 0 .. n_samples // 1024 - 1: the chunks
    whose right context those samples cover (decodable-online-looped.cc:56-84), no flush."""
    _, R = orc.nnet.context()
    out = []
    for j in range(n_samples // TICK):
        fr = orc.mfcc.num_frames(TICK * (j + 1))
        t1 = max(0, fr - R) // orc.chunk * orc.chunk
        out.append((t1 + orc.fsf - 1) // orc.fsf)
    return out


class TickOracle:
    """FinalRelativeCost() and TrailingSilenceLength() (online-endpoint.cc:109-126) of the oracle's search over the first n rows of
    `ll`: the oracle's lattice with lattice_beam = 1e9 and the graph's final weights removed keeps every token of every frame
    (tests/test_gpu_stream_partial.py: _oracle_best); a forward pass over it gives every last-frame token's best cost and back
    pointer, and following the lattice's arcs through HCLG from the start state gives the token's graph state."""

    def __init__(self, orc, id2phone: np.ndarray):
        self.orc, self.id2phone = orc, id2phone
        self.fst_nofinal = copy.copy(orc.fst)
        self.fst_nofinal.final = np.full_like(np.asarray(orc.fst.final), np.inf)
        self.final = np.asarray(orc.fst.final, np.float32)
        f = orc.fst
        self._ab, self._il, self._ol = np.asarray(f.arc_begin), np.asarray(f.ilabel), np.asarray(f.olabel)
        self._w, self._ns = np.asarray(f.weight, np.float32), np.asarray(f.nextstate)
        self._arcs_of: Dict[int, dict] = {}
        self._memo: Dict[int, tuple] = {}

    def _next(self, h: int, il: int, ol: int, g: float) -> int:
        table = self._arcs_of.get(h)
        if table is None:
            table = {}
            for a in range(int(self._ab[h]), int(self._ab[h + 1])):
                table.setdefault((int(self._il[a]), int(self._ol[a]), float(self._w[a])), set()).add(int(self._ns[a]))
            self._arcs_of[h] = table
        dst = table[(il, ol, g)]
        assert len(dst) == 1, "two graph arcs of one state with the same labels and weight: the lattice does not say which was taken"
        return next(iter(dst))

    def frontier(self, ll: np.ndarray, n: int):
        """-> (graph state, cost, back-pointer chain of input labels last first) per last-frame token, as arrays / a function."""
        if n in self._memo:
            return self._memo[n]
        self._memo.clear()                               # (one lattice at a time: they are large)
        from oracle import pipeline
        opts = dict(self.orc.opts, lattice_beam=1e9)
        l, _ = pipeline.decode(self.fst_nofinal, self.orc.id2pdf, ll[:n], **opts)
        ns = l.num_states
        out_arcs: List[List[int]] = [[] for _ in range(ns)]
        for a in range(l.num_arcs):
            out_arcs[int(l.src[a])].append(a)
        topo = np.argsort(pipeline.lat._topo_order(l, out_arcs))      # (_topo_order gives each state's rank)
        alpha = np.full(ns, np.inf)
        hstate = np.full(ns, -1, np.int64)
        back = np.full(ns, -1, np.int64)
        alpha[l.start], hstate[l.start] = 0.0, int(self.orc.fst.start)
        for s in topo:
            s = int(s)
            if not np.isfinite(alpha[s]):
                continue
            for a in out_arcs[s]:
                d = int(l.dst[a])
                h = self._next(int(hstate[s]), int(l.ilabel[a]), int(l.olabel[a]), float(np.float32(l.graph[a])))
                assert hstate[d] in (-1, h)
                hstate[d] = h
                c = alpha[s] + float(l.graph[a]) + float(l.acoustic[a])
                if c < alpha[d]:
                    alpha[d], back[d] = c, a
        last = np.nonzero((l.state_frame == n) & np.isfinite(alpha))[0]
        self._memo[n] = (l, alpha, hstate, back, last)
        return self._memo[n]

    def values(self, ll: np.ndarray, n: int, silence_phones) -> Tuple[int, float, float]:
        """-> (trailing silence frames, final relative cost, margin): margin = how far the second-best frontier token is behind the
        best one (a tie within float rounding could start the walk from another token)."""
        l, alpha, hstate, back, last = self.frontier(ll, n)
        if len(last) == 0:
            return 0, float("inf"), float("inf")
        sil = set(int(p) for p in silence_phones)
        costs = alpha[last]
        k = np.lexsort((hstate[last], costs))
        best = int(last[k[0]])
        margin = float(costs[k[1]] - costs[k[0]]) if len(last) > 1 else float("inf")
        with_final = float(np.min(costs + self.final[hstate[last]].astype(np.float64)))
        rel = with_final - float(alpha[best]) if np.isfinite(with_final) else float("inf")
        count, s = 0, best
        while back[s] >= 0:
            a = int(back[s])
            il = int(l.ilabel[a])
            if il != 0:
                if int(self.id2phone[il]) in sil:
                    count += 1
                else:
                    break
            s = int(l.src[a])
        return count, rel, margin

    def best_phones(self, ll: np.ndarray, n: int) -> List[int]:
        """The phones of the best frontier token's path, last frame first (for --explore)."""
        l, alpha, hstate, back, last = self.frontier(ll, n)
        if len(last) == 0:
            return []
        k = np.lexsort((hstate[last], alpha[last]))
        s, out = int(last[k[0]]), []
        while back[s] >= 0:
            a = int(back[s])
            if int(l.ilabel[a]) != 0:
                out.append(int(self.id2phone[int(l.ilabel[a])]))
            s = int(l.src[a])
        return out
