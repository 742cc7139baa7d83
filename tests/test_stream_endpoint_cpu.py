"""Endpoint detection on streams (rs_streams_endpoint / rs_streams_finalize), the parts that need no GPU: the C declarations and
exports, the options of online.conf, the five rules on the host against a restatement of RuleActivated in numpy.float32, and the
control flow of KaldiNnet3StreamTranscriber.async_transcribe_until_endpoint on a stand-in stream."""
import asyncio
import inspect
import re
import shutil

import numpy as np
import pytest

from tests.cases import GOLDEN

HEADER = GOLDEN.parent.parent / "include" / "rhasspy_speech_hip.h"
INF = float("inf")
# online-endpoint.h:152-157: (must_contain_nonsilence, min_trailing_silence, max_relative_cost, min_utterance_length)
DEFAULT_RULES = [(0, 5.0, INF, 0.0), (1, 0.5, 2.0, 0.0), (1, 1.0, 8.0, 0.0), (1, 2.0, INF, 0.0), (0, 0.0, INF, 20.0)]


def _rules(o):
    return [(r.must_contain_nonsilence, r.min_trailing_silence, r.max_relative_cost, r.min_utterance_length) for r in o.rule]


def test_header_declares_endpoint_entry_points_and_lib_exports_them():
    from rhasspy_speech_amd import _lib
    text = re.sub(r"\s+", " ", HEADER.read_text())
    for decl in [
        "int rs_default_endpoint_opts(rs_endpoint_opts *opts);",
        "int rs_model_endpoint_opts(const rs_model *model, rs_endpoint_opts *opts);",
        "int rs_endpoint_rule_fired(const rs_endpoint_opts *opts, int32_t num_frames_decoded, int32_t trailing_silence_frames, "
        "float frame_shift_seconds, float final_relative_cost);",
        "int rs_streams_endpoint(rs_stream *const *streams, int32_t n_streams, const rs_endpoint_opts *opts, rs_endpoint_status *out);",
        "int rs_stream_endpoint(rs_stream *stream, const rs_endpoint_opts *opts, rs_endpoint_status *out);",
        "int rs_streams_finalize(rs_stream *const *streams, int32_t n_streams, int32_t nbest, float lattice_acoustic_scale, rs_result **out);",
    ]:
        assert decl in text, decl
    for field in ["must_contain_nonsilence", "min_trailing_silence", "max_relative_cost", "min_utterance_length", "int32_t detected;",
                  "int32_t num_frames_decoded;", "int32_t trailing_silence_frames;", "float final_relative_cost;", "float frame_shift_seconds;"]:
        assert field in text, field
    assert re.search(r"typedef struct rs_endpoint_rule \{", text) and re.search(r"typedef struct rs_endpoint_opts \{", text)
    assert re.search(r"typedef struct rs_endpoint_status \{", text)
    for sym in ["rs_default_endpoint_opts", "rs_model_endpoint_opts", "rs_endpoint_rule_fired", "rs_streams_endpoint", "rs_stream_endpoint",
                "rs_streams_finalize", "rs_stream_finalize"]:
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym), sym
    assert hasattr(_lib.Stream, "endpoint") and hasattr(_lib.Stream, "finalize") and hasattr(_lib.Model, "endpoint_opts")
    assert callable(_lib.endpoint_streams) and callable(_lib.finalize_streams) and issubclass(_lib.EndpointOpts, object)
    # rs_decode_opts keeps its layout: the endpoint options travel in a struct of their own
    assert "endpoint" not in [f[0] for f in _lib.DecodeOpts._fields_]


def test_default_endpoint_opts_are_the_references():
    from rhasspy_speech_amd import _lib
    o = _lib.default_endpoint_opts()
    assert _rules(o) == DEFAULT_RULES
    assert o.silence_phones == b""


def _model_with_conf(case_cache, tmp_path, extra_lines):
    model_dir, graph_dir, _, _ = case_cache("tiny_u0")
    dst = tmp_path / "model_dir"
    shutil.copytree(model_dir, dst)
    conf = dst / "model" / "online" / "conf" / "online.conf"
    conf.write_text(conf.read_text().replace(str(model_dir), str(dst)) + "".join(l + "\n" for l in extra_lines))
    for sub in conf.parent.glob("*.conf"):
        sub.write_text(sub.read_text().replace(str(model_dir), str(dst)))
    return dst, graph_dir


def test_model_endpoint_opts_come_from_online_conf(case_cache, tmp_path):
    from rhasspy_speech_amd import _lib
    plain = _lib.Model(*case_cache("tiny_u0")[:2]).endpoint_opts()
    assert _rules(plain) == DEFAULT_RULES and plain.silence_phones == b"1"      # synth.py writes --endpoint.silence-phones=1
    md, gd = _model_with_conf(case_cache, tmp_path, [
        "--endpoint.silence-phones=1:2:7", "--endpoint.rule1.min-trailing-silence=3.25", "--endpoint.rule2.must-contain-nonsilence=false",
        "--endpoint.rule2.max-relative-cost=1.5", "--endpoint.rule3.min-utterance-length=0.75", "--endpoint.rule4.max-relative-cost=inf",
        "--endpoint.rule5.min-utterance-length=12", "--endpoint.rule5.must-contain-nonsilence=true", "--endpoint.rule5.min-utterance-length=9.5"])
    o = _lib.Model(md, gd).endpoint_opts()
    assert o.silence_phones == b"1:2:7"
    assert _rules(o) == [(0, 3.25, INF, 0.0), (0, 0.5, 1.5, 0.0), (1, 1.0, 8.0, 0.75), (1, 2.0, INF, 0.0), (1, 0.0, INF, 9.5)]


@pytest.mark.parametrize("line,needle", [("--endpoint.rule2.min-trailing-silence=abc", "Invalid floating-point option"),
                                         ("--endpoint.rule1.must-contain-nonsilence=maybe", "Invalid format for boolean argument"),
                                         ("--endpoint.rule6.min-trailing-silence=1", "Invalid option --endpoint.rule6"),
                                         ("--endpoint.silence-phones=" + "1:" * 2100 + "1", "longer than")])
def test_bad_endpoint_values_do_not_fail_the_load_but_the_first_endpoint_call(case_cache, tmp_path, line, needle):
    from rhasspy_speech_amd import _lib
    md, gd = _model_with_conf(case_cache, tmp_path, [line])
    model = _lib.Model(md, gd)                     # loads, as it did when these lines were skipped
    with pytest.raises(_lib.RsError, match=re.escape(needle)):
        model.endpoint_opts()


def _rule_activated(rule, trailing_silence, relative_cost, utterance_length):
    """RuleActivated, online-endpoint.cc:26-44, in BaseFloat."""
    must, min_sil, max_cost, min_len = rule
    contains_nonsilence = utterance_length > trailing_silence
    return bool((contains_nonsilence or not must) and trailing_silence >= np.float32(min_sil) and relative_cost <= np.float32(max_cost)
                and utterance_length >= np.float32(min_len))


def _endpoint_detected(rules, frames, sil, shift, cost):
    """EndpointDetected, online-endpoint.cc:46-72: the number of the first rule that fires, 0 if none does."""
    shift, cost = np.float32(shift), np.float32(cost)
    utterance_length, trailing_silence = np.float32(frames) * shift, np.float32(sil) * shift
    for k, r in enumerate(rules):
        if _rule_activated(r, trailing_silence, cost, utterance_length):
            return k + 1
    return 0


def _opts_from(rules):
    from rhasspy_speech_amd import _lib
    o = _lib.default_endpoint_opts()
    for k, r in enumerate(rules):
        o.rule[k].must_contain_nonsilence, o.rule[k].min_trailing_silence, o.rule[k].max_relative_cost, o.rule[k].min_utterance_length = r
    return o


def test_rule_evaluation_equals_rule_activated_in_float32():
    from rhasspy_speech_amd import _lib
    rng = np.random.default_rng(5)
    n_fired = [0] * 6
    for trial in range(6000):
        if trial % 3 == 0:
            rules = DEFAULT_RULES
        else:
            rules = [(int(rng.integers(0, 2)), float(np.float32(rng.choice([0.0, 0.3, 0.5, 1.0, 2.0, 5.0]) * rng.uniform(0.5, 1.5))),
                      float(np.float32(rng.choice([INF, 0.0, 2.0, 8.0, 30.0]))), float(np.float32(rng.choice([0.0, 0.0, 1.0, 20.0]))))
                     for _ in range(5)]
        shift = float(np.float32(rng.choice([0.01, 0.03, 0.02, 0.0125])))
        frames = int(rng.integers(0, 3000))
        sil = int(rng.integers(0, frames + 1)) if rng.random() < 0.8 else frames
        cost = float(np.float32(rng.choice([INF, 0.0, 2.0, 8.0, float(rng.uniform(0, 12))])))
        want = _endpoint_detected(rules, frames, sil, shift, cost)
        got = _lib.endpoint_rule_fired(_opts_from(rules), frames, sil, shift, cost)
        assert got == want, (rules, frames, sil, shift, cost)
        n_fired[want] += 1
    assert all(n > 50 for n in n_fired), n_fired      # every outcome was exercised
    # the edges: all silence, nothing decoded, no final state reached, exact thresholds (0.5 s = 50 frames of 10 ms in float)
    o = _lib.default_endpoint_opts()
    for frames, sil, shift, cost in [(600, 600, 0.01, 0.0), (499, 499, 0.01, 0.0), (500, 500, 0.01, INF), (0, 0, 0.01, INF), (0, 0, 0.03, 0.0),
                                     (300, 50, 0.01, 2.0), (300, 49, 0.01, 2.0), (300, 50, 0.01, np.nextafter(np.float32(2.0), np.float32(3.0))),
                                     (300, 100, 0.01, 8.0), (300, 99, 0.01, 8.0), (300, 200, 0.01, INF), (300, 199, 0.01, INF),
                                     (2000, 0, 0.01, INF), (1999, 0, 0.01, INF), (667, 0, 0.03, INF), (666, 0, 0.03, INF), (17, 17, 0.03, 0.0)]:
        assert _lib.endpoint_rule_fired(o, frames, sil, shift, float(cost)) == _endpoint_detected(DEFAULT_RULES, frames, sil, shift, cost), \
            (frames, sil, shift, cost)
    assert _lib.endpoint_rule_fired(o, 600, 600, 0.01, 0.0) == 1 and _lib.endpoint_rule_fired(o, 300, 50, 0.01, 2.0) == 2
    assert _lib.endpoint_rule_fired(o, 300, 100, 0.01, 8.0) == 3 and _lib.endpoint_rule_fired(o, 300, 200, 0.01, INF) == 4
    assert _lib.endpoint_rule_fired(o, 2000, 0, 0.01, INF) == 5 and _lib.endpoint_rule_fired(o, 0, 0, 0.01, INF) == 0


# ---------------------------------------------------------------------------------------------- the transcriber's control flow
class _Res:
    def __init__(self, words=None, text=b""):
        self._words, self._text = words or [], text

    def words(self, utt, k=0):
        return list(self._words)

    def text(self, utt, key="utt"):
        return self._text

    def close(self):
        pass


class _Status:
    def __init__(self, detected):
        self.detected = detected


class _StubStream:
    """Stands in for _lib.Stream: endpoint() after the k-th accept returns DETECT[k] (0 beyond the script)."""
    DETECT = []
    log = []

    def __init__(self, model):
        self.n = 0

    def accept(self, chunk):
        self.n += 1
        _StubStream.log.append(("accept", len(chunk)))

    def advance(self):
        _StubStream.log.append(("advance",))

    def partial(self):
        _StubStream.log.append(("partial",))
        return _Res([3] if self.n < 3 else [3, 5])

    def endpoint(self, opts=None):
        _StubStream.log.append(("endpoint", opts))
        return _Status(self.DETECT[self.n - 1] if self.n <= len(self.DETECT) else 0)

    def finish(self, nbest, scale):
        _StubStream.log.append(("finish", nbest, scale))
        return _Res(text=b"utt-1 4 6 \n")

    def finalize(self, nbest, scale):
        _StubStream.log.append(("finalize", nbest, scale))
        return _Res(text=b"utt-1 3 5 \n")

    def close(self):
        pass


def _transcriber(monkeypatch, tmp_path):
    from rhasspy_speech_amd import transcribe_stream
    monkeypatch.setattr(transcribe_stream._lib, "Stream", _StubStream)
    tr = transcribe_stream.KaldiNnet3StreamTranscriber(tmp_path, tmp_path)
    tr._model = object()
    tr._words = {3: "turn", 4: "what", 5: "on", 6: "time"}
    return tr


class _Audio:
    """An async iterator that counts what was pulled from it."""

    def __init__(self, n):
        self.n, self.pulled = n, 0

    def __aiter__(self):
        return self

    async def __anext__(self):
        if self.pulled >= self.n:
            raise StopAsyncIteration
        self.pulled += 1
        return b"" if self.pulled == 2 else bytes(2 * (100 + self.pulled))      # (an empty chunk is skipped, like in async_transcribe)


def test_until_endpoint_stops_pulling_audio_and_finalizes(monkeypatch, tmp_path):
    tr = _transcriber(monkeypatch, tmp_path)
    _StubStream.DETECT, _StubStream.log = [0, 0, 0, 3, 2], []
    audio = _Audio(12)
    opts = object()
    got = asyncio.run(tr.async_transcribe_until_endpoint(audio, tmp_path, endpoint_opts=opts))
    assert audio.pulled == 5                       # 4 accepted chunks + the empty one; nothing after the detection
    assert [e[0] for e in _StubStream.log] == ["accept", "endpoint"] * 4 + ["finalize"]
    assert all(e[1] is opts for e in _StubStream.log if e[0] == "endpoint")
    assert _StubStream.log[-1] == ("finalize", 1, tr.acoustic_scale)
    assert got == ["turn on"] and tr.last_endpoint_rule == 3


def test_until_endpoint_falls_back_to_finish_when_the_audio_ends_first(monkeypatch, tmp_path):
    tr = _transcriber(monkeypatch, tmp_path)
    _StubStream.DETECT, _StubStream.log = [], []
    tr.last_endpoint_rule = 4
    audio = _Audio(6)
    seen = []
    got = asyncio.run(tr.async_transcribe_until_endpoint(audio, tmp_path, nbest=2, on_partial=seen.append))
    assert audio.pulled == 6
    assert [e[0] for e in _StubStream.log] == ["accept", "partial", "endpoint"] * 5 + ["finish"]
    assert _StubStream.log[-1] == ("finish", 2, tr.acoustic_scale)
    assert got == ["what time"] and tr.last_endpoint_rule == 0 and seen == ["turn", "turn on"]
    _StubStream.log = []
    assert asyncio.run(tr.async_transcribe(_Audio(6), tmp_path)) == got
    assert [e[0] for e in _StubStream.log] == ["accept", "advance"] * 5 + ["finish"]


def test_existing_transcriber_signatures_are_untouched():
    from rhasspy_speech_amd.transcribe_stream import KaldiNnet3StreamTranscriber
    sig = inspect.signature(KaldiNnet3StreamTranscriber.async_transcribe)
    assert list(sig.parameters)[1:] == ["audio_stream", "lang_dir", "nbest", "max_fuzzy_cost", "require_fuzzy"]
    assert [sig.parameters[k].default for k in ("nbest", "max_fuzzy_cost", "require_fuzzy")] == [1, None, False]
    sig = inspect.signature(KaldiNnet3StreamTranscriber.async_transcribe_with_partials)
    assert list(sig.parameters)[1:] == ["audio_stream", "lang_dir", "on_partial", "nbest", "max_fuzzy_cost", "require_fuzzy"]
    sig = inspect.signature(KaldiNnet3StreamTranscriber.async_transcribe_until_endpoint)
    assert list(sig.parameters)[1:] == ["audio_stream", "lang_dir", "nbest", "max_fuzzy_cost", "require_fuzzy", "on_partial", "endpoint_opts"]
    assert [sig.parameters[k].default for k in ("nbest", "max_fuzzy_cost", "require_fuzzy", "on_partial", "endpoint_opts")] == [1, None, False, None, None]
