"""Partial results of streams (rs_streams_partial / rs_stream_partial), the parts that need no GPU: the C declarations and exports,
and the control flow of KaldiNnet3StreamTranscriber.async_transcribe_with_partials on a stand-in stream."""
import asyncio
import inspect
import re

from tests.cases import GOLDEN

HEADER = GOLDEN.parent.parent / "include" / "rhasspy_speech_hip.h"


def test_header_declares_partial_entry_points_and_lib_exports_them():
    from rhasspy_speech_amd import _lib
    text = HEADER.read_text()
    assert re.search(r"int rs_streams_partial\(rs_stream \*const \*streams, int32_t n_streams, rs_result \*\*out\);", text)
    assert re.search(r"int rs_stream_partial\(rs_stream \*stream, rs_result \*\*out\);", text)
    assert "rs_streams_partial" in _lib.EXPORTS and "rs_stream_partial" in _lib.EXPORTS
    assert hasattr(_lib.Stream, "partial") and callable(_lib.partial_streams)


class _Res:
    def __init__(self, words=None, text=b""):
        self._words, self._text = words or [], text

    def words(self, utt, k=0):
        return list(self._words)

    def text(self, utt, key="utt"):
        return self._text

    def close(self):
        pass


class _StubStream:
    """Stands in for _lib.Stream: partial() after the k-th accept returns SCRIPT[k]; finish() the text of the last one."""
    SCRIPT = [[], [], [3], [3], [3, 5], [3, 5], [4], [4, 6], [4, 6]]
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
        return _Res(self.SCRIPT[self.n - 1])

    def finish(self, nbest, scale):
        _StubStream.log.append(("finish", nbest, scale))
        return _Res(text=b"utt-1 4 6 \n")

    def close(self):
        pass


def _transcriber(monkeypatch, tmp_path):
    from rhasspy_speech_amd import transcribe_stream
    monkeypatch.setattr(transcribe_stream._lib, "Stream", _StubStream)
    tr = transcribe_stream.KaldiNnet3StreamTranscriber(tmp_path, tmp_path)
    tr._model = object()
    tr._words = {3: "turn", 4: "what", 5: "on", 6: "time"}
    return tr


async def _chunks(n):
    for k in range(n):
        yield bytes(2 * (100 + k))
    yield b""          # (an empty chunk is skipped, like in async_transcribe)


def test_partials_fire_only_when_the_words_change_and_the_result_is_async_transcribes(monkeypatch, tmp_path):
    tr = _transcriber(monkeypatch, tmp_path)
    n = len(_StubStream.SCRIPT)
    _StubStream.log = []
    plain = asyncio.run(tr.async_transcribe(_chunks(n), tmp_path))
    assert [e[0] for e in _StubStream.log] == ["accept", "advance"] * n + ["finish"]
    _StubStream.log = []
    seen = []
    got = asyncio.run(tr.async_transcribe_with_partials(_chunks(n), tmp_path, seen.append))
    assert [e[0] for e in _StubStream.log] == ["accept", "partial"] * n + ["finish"]
    assert seen == ["turn", "turn on", "what", "what time"]
    assert got == plain == ["what time"]


def test_partial_text_is_made_like_the_final_text(monkeypatch, tmp_path):
    from rhasspy_speech_amd.meta import encode_meta
    tr = _transcriber(monkeypatch, tmp_path)
    tr._words[9] = encode_meta('{"text": "on", "list": null}')
    assert tr._partial_text([3, 9]) == "turn on"
    assert tr._partial_text([]) == ""


def test_async_transcribe_signature_is_untouched():
    from rhasspy_speech_amd.transcribe_stream import KaldiNnet3StreamTranscriber
    sig = inspect.signature(KaldiNnet3StreamTranscriber.async_transcribe)
    assert list(sig.parameters)[1:] == ["audio_stream", "lang_dir", "nbest", "max_fuzzy_cost", "require_fuzzy"]
    sig = inspect.signature(KaldiNnet3StreamTranscriber.async_transcribe_with_partials)
    assert list(sig.parameters)[1:] == ["audio_stream", "lang_dir", "on_partial", "nbest", "max_fuzzy_cost", "require_fuzzy"]
    assert [sig.parameters[k].default for k in ("nbest", "max_fuzzy_cost", "require_fuzzy")] == [1, None, False]
