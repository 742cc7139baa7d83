"""Transcribe an audio stream on an MI355X.

Same public surface as rhasspy_speech/transcribe_stream.py:18-129: `KaldiNnet3StreamTranscriber.async_transcribe`
consumes an async iterable of raw s16le mono chunks at the model's sampling rate (the bytes the reference writes to the stdin of
`online2-cli-nnet3-decode-faster`, :76-82; `samp_freq`, the binary's --samp-freq, says which: 16 kHz unless given, 8000 for a
telephone model) and returns the decoded texts.  The library re-chunks to the binary's
fixed 1024-sample ticks, so -- like the reference -- the result does not depend on how the caller slices the audio.
`async_transcribe_with_partials` also reports the best path so far as the audio arrives (the "temporary transcript" of
online2-tcp-nnet3-decode-faster.cc:302-318), and returns what `async_transcribe` returns.
`async_transcribe_until_endpoint` also asks, after every chunk, whether the reference's endpointing rules fire
(online2/online-endpoint.cc; rs_stream_endpoint) and, when they do, stops reading audio and finalizes the frames decoded so far
like online2-wav-nnet3-latgen-faster.cc:270-278 does.
`async_transcribe_continuous` keeps listening after an endpoint: one transcript per utterance, every utterance after the first
opened with the speaker adaptation state of the ones before (online2-wav-nnet3-latgen-faster.cc:203-205, 220-221, 287-288).
"""
from __future__ import annotations

import asyncio
import logging
from collections.abc import AsyncIterable
from pathlib import Path
from typing import AsyncIterator, Callable, List, Optional, Union

from . import _lib
from .meta import decode_meta, int2sym, read_words_txt, texts_from_int2sym
from .transcribe_util import get_fuzzy_text
from .tools import KaldiTools

_LOGGER = logging.getLogger(__name__)


class KaldiNnet3StreamTranscriber:
    def __init__(
        self,
        model_dir: Union[str, Path],
        graph_dir: Union[str, Path],
        tools: Optional[KaldiTools] = None,
        max_active: int = 7000,
        lattice_beam: float = 8.0,
        acoustic_scale: float = 1.0,
        beam: float = 24.0,
        device_id: int = 0,
        samp_freq: float = 16000.0,
    ):
        self.model_dir = Path(model_dir)
        self.graph_dir = Path(graph_dir)
        self.tools = tools
        self.max_active = max_active
        self.lattice_beam = lattice_beam
        self.acoustic_scale = acoustic_scale
        self.beam = beam
        self.device_id = device_id
        self.samp_freq = samp_freq      # online2-cli-nnet3-decode-faster.cc:67-70 (the reference's Python never passes it)
        self._model: Optional[_lib.Model] = None
        self._words = None
        self._lat_model: Optional[_lib.Model] = None      # the same files, results keep their lattices (rescoring path)
        self._rescorers = {}
        self._rate_error: Optional[str] = None      # what rs_model_check_sample_rate said about samp_freq when the model was loaded
        self.last_endpoint_rule = 0      # async_transcribe_until_endpoint: the rule (1..5) that ended the last call, 0 = the audio ended first
        self.last_adaptation: Optional[_lib.Adaptation] = None      # async_transcribe_continuous: the speaker's state after the last utterance

    def _ensure_loaded(self) -> _lib.Model:
        if self._model is None:
            opts = _lib.default_opts(max_active=self.max_active, lattice_beam=self.lattice_beam, beam=self.beam,
                                     acoustic_scale=1.0, device_id=self.device_id)
            self._model = self._load_model(opts)
            self._words = read_words_txt(self.graph_dir / "words.txt")
        return self._model

    def _load_model(self, opts) -> _lib.Model:
        model = _lib.Model(self.model_dir, self.graph_dir, opts)
        try:
            model.check_sample_rate(self.samp_freq)
        except _lib.RsError as e:
            self._rate_error = str(e)
        return model

    def _open_stream(self, model: _lib.Model, adaptation=None) -> _lib.Stream:
        """A stream on `model`, refused before any audio when `samp_freq` is not the model's rate: the binary hands --samp-freq to
        AcceptWaveform with the first block (:148) and ends with "Sampling frequency mismatch, expected ..., got ..."."""
        if self._rate_error is not None:
            raise RuntimeError(f"Unexpected error running command online2-cli-nnet3-decode-faster (HIP): {self._rate_error}")
        return _lib.Stream(model) if adaptation is None else _lib.Stream(model, adaptation=adaptation)

    @staticmethod
    def _accept_and_advance(stream, chunk) -> None:
        stream.accept(chunk)
        stream.advance()

    @staticmethod
    def _accept_and_partial(stream, chunk) -> List[int]:
        stream.accept(chunk)
        res = stream.partial()
        try:
            return res.words(0)
        finally:
            res.close()

    @staticmethod
    def _accept_and_endpoint(stream, chunk, want_partial: bool, endpoint_opts):
        """One chunk of async_transcribe_until_endpoint: -> (the partial's words or None, the rule that fired or 0)."""
        stream.accept(chunk)
        words = None
        if want_partial:
            res = stream.partial()
            try:
                words = res.words(0)
            finally:
                res.close()
        return words, int(stream.endpoint(endpoint_opts).detected)

    def _partial_text(self, words: List[int]) -> str:
        """A partial's words as the final text is made of them: int2sym, then the meta words decoded (no fuzzy match)."""
        line = int2sym(("utt-1 " + " ".join(str(w) for w in words) + "\n").encode(), self._words)
        parts = line.strip().split(maxsplit=1)
        return decode_meta(parts[1]) if len(parts) > 1 else ""

    async def async_transcribe(
        self,
        audio_stream: AsyncIterable[Optional[bytes]],
        lang_dir: Union[str, Path],
        nbest: int = 1,
        max_fuzzy_cost: Optional[float] = None,
        require_fuzzy: bool = False,
    ) -> List[str]:
        return await self._transcribe(audio_stream, lang_dir, nbest, max_fuzzy_cost, require_fuzzy, None)

    async def async_transcribe_with_partials(
        self,
        audio_stream: AsyncIterable[Optional[bytes]],
        lang_dir: Union[str, Path],
        on_partial: Callable[[str], None],
        nbest: int = 1,
        max_fuzzy_cost: Optional[float] = None,
        require_fuzzy: bool = False,
    ) -> List[str]:
        """`async_transcribe`, and after every chunk the best path so far (rs_stream_partial: no final costs): `on_partial(text)` is
        called whenever its words differ from the last ones reported (none before the first word).  Returns exactly what
        `async_transcribe` returns for the same audio."""
        return await self._transcribe(audio_stream, lang_dir, nbest, max_fuzzy_cost, require_fuzzy, on_partial)

    async def async_transcribe_until_endpoint(
        self,
        audio_stream: AsyncIterable[Optional[bytes]],
        lang_dir: Union[str, Path],
        nbest: int = 1,
        max_fuzzy_cost: Optional[float] = None,
        require_fuzzy: bool = False,
        on_partial: Optional[Callable[[str], None]] = None,
        endpoint_opts=None,
    ) -> List[str]:
        """`async_transcribe` that stops at the speaker's end: after every accepted chunk the stream is asked for an endpoint
        (rs_stream_endpoint; `endpoint_opts` None = the model's online.conf over the reference's defaults).  On a detection no more
        audio is taken from `audio_stream`, the frames decoded so far are finalized (rs_stream_finalize: no flush of the feature tail)
        and post-processed exactly like `async_transcribe` does; if the audio ends first, this IS `async_transcribe`.  With
        `on_partial`, partials are reported as by `async_transcribe_with_partials`.  `self.last_endpoint_rule` holds the rule (1..5)
        that fired, 0 if none did."""
        return await self._transcribe(audio_stream, lang_dir, nbest, max_fuzzy_cost, require_fuzzy, on_partial, until_endpoint=True,
                                      endpoint_opts=endpoint_opts)

    async def _transcribe(self, audio_stream, lang_dir, nbest, max_fuzzy_cost, require_fuzzy, on_partial, until_endpoint=False,
                          endpoint_opts=None) -> List[str]:
        lang_dir = Path(lang_dir)
        stream = self._open_stream(self._ensure_loaded())
        loop = asyncio.get_running_loop()
        reported: List[int] = []
        fired = 0
        if until_endpoint:
            self.last_endpoint_rule = 0
        try:
            async for chunk in audio_stream:
                if chunk and until_endpoint:
                    words, fired = await loop.run_in_executor(None, self._accept_and_endpoint, stream, chunk, on_partial is not None,
                                                              endpoint_opts)
                    if words is not None and words != reported:
                        reported = words
                        on_partial(self._partial_text(words))
                    if fired:      # online2-wav-nnet3-latgen-faster.cc:270-274: break out of the chunk loop
                        self.last_endpoint_rule = fired
                        _LOGGER.debug("Endpoint detected by rule %d", fired)
                        break
                    continue
                if chunk:
                    # the reference writes the chunk to the decoder's stdin and awaits the drain (transcribe_stream.py:73-76) while the
                    # decoder decodes as it reads; here: hand the samples over and let the device do what they make possible (MFCC,
                    # iVector, nnet chunks, search) -- in the executor, so the event loop is not held while the library plans and
                    # issues the advance (the calls release the GIL)
                    if on_partial is None:
                        await loop.run_in_executor(None, self._accept_and_advance, stream, chunk)
                        continue
                    words = await loop.run_in_executor(None, self._accept_and_partial, stream, chunk)
                    if words != reported:
                        reported = words
                        on_partial(self._partial_text(words))
            _LOGGER.debug("Stream ended")
            try:
                res = await loop.run_in_executor(None, stream.finalize if fired else stream.finish, nbest, self.acoustic_scale)
                nbest_stdout = res.text(0, "utt")
            except _lib.RsError as e:
                # The reference never checks the decoder's exit status (transcribe_stream.py:82) and then fails in
                # lattice-to-nbest on the missing lattice; surface the decoder's message instead.
                raise RuntimeError(f"Unexpected error running command online2-cli-nnet3-decode-faster (HIP): {e}") from e
        finally:
            stream.close()
        return self._texts(nbest_stdout, lang_dir, max_fuzzy_cost, require_fuzzy)

    def _texts(self, nbest_stdout: bytes, lang_dir: Path, max_fuzzy_cost, require_fuzzy) -> List[str]:
        """The n-best list of one utterance -> its texts (the post-processing every entry point shares)."""
        int2sym_stdout = int2sym(nbest_stdout, self._words)
        _LOGGER.debug("nbest: %s", int2sym_stdout)
        fuzzy_result = get_fuzzy_text(nbest_stdout, lang_dir)      # transcribe_stream.py:111-116
        if fuzzy_result is not None:
            text, cost = fuzzy_result
            _LOGGER.debug("Fuzzy cost: %s", cost)
            if cost <= max_fuzzy_cost:       # (like the reference, a TypeError when max_fuzzy_cost is None)
                return [decode_meta(text)]
        if require_fuzzy:
            return []
        return texts_from_int2sym(int2sym_stdout)

    # ---- one speaker, utterance after utterance
    @staticmethod
    def _accept_tick(stream, tick, endpoint_opts) -> int:
        stream.accept(tick)
        return int(stream.endpoint(endpoint_opts).detected)

    @staticmethod
    def _end_utterance(stream, fired: bool, nbest: int, acoustic_scale: float):
        """-> (the n-best list, the speaker's state after the utterance)"""
        res = (stream.finalize if fired else stream.finish)(nbest, acoustic_scale)
        try:
            return res.text(0, "utt"), stream.adaptation()
        finally:
            res.close()

    async def async_transcribe_continuous(
        self,
        audio_stream: AsyncIterable[Optional[bytes]],
        lang_dir: Union[str, Path],
        nbest: int = 1,
        max_fuzzy_cost: Optional[float] = None,
        require_fuzzy: bool = False,
        endpoint_opts=None,
        adaptation: Optional[_lib.Adaptation] = None,
    ) -> AsyncIterator[List[str]]:
        """An async generator over ONE speaker's audio: yields what `async_transcribe` returns, once per utterance.  The audio is
        cut into the 1024-sample ticks of the stream binary; after every tick the stream is asked for an endpoint
        (rs_stream_endpoint, `endpoint_opts` None = the model's).  On a detection the utterance is finalized at that tick
        (rs_stream_finalize), its adaptation state is taken (rs_stream_adaptation) and the next utterance is opened with it
        (rs_stream_open_adapted); audio that arrived after the deciding tick goes to the next utterance, in order.  The last
        utterance ends with the audio (rs_stream_finish: the feature tail is flushed); nothing is yielded for an utterance without
        audio.  `adaptation`: the speaker's state from an earlier call or process (None = a new speaker); `self.last_adaptation` holds
        the state after the last utterance yielded."""
        lang_dir = Path(lang_dir)
        model = self._ensure_loaded()
        loop = asyncio.get_running_loop()
        tick_bytes = 2 * 1024
        state = adaptation
        stream = self._open_stream(model, adaptation=state)
        pending = bytearray()
        fed = 0                # bytes the current utterance has got

        async def end(fired: bool):
            nonlocal stream, state, fed
            try:
                nbest_stdout, state = await loop.run_in_executor(None, self._end_utterance, stream, fired, nbest, self.acoustic_scale)
            except _lib.RsError as e:
                raise RuntimeError(f"Unexpected error running command online2-cli-nnet3-decode-faster (HIP): {e}") from e
            finally:
                stream.close()
            self.last_adaptation = state
            stream, fed = self._open_stream(model, adaptation=state), 0
            return self._texts(nbest_stdout, lang_dir, max_fuzzy_cost, require_fuzzy)

        try:
            async for chunk in audio_stream:
                if not chunk:
                    continue
                pending += chunk
                while len(pending) >= tick_bytes:
                    tick = bytes(pending[:tick_bytes])
                    del pending[:tick_bytes]
                    fed += tick_bytes
                    fired = await loop.run_in_executor(None, self._accept_tick, stream, tick, endpoint_opts)
                    if fired:
                        _LOGGER.debug("Endpoint detected by rule %d", fired)
                        yield await end(True)
            if pending:
                await loop.run_in_executor(None, stream.accept, bytes(pending))
                fed += len(pending)
            if fed:
                yield await end(False)
        finally:
            stream.close()

    # ---- rescoring path (transcribe_stream.py:131-274): stream through the old graph, re-rank the lattice with a NEW lexicon + LM
    async def async_transcribe_rescore(
        self,
        audio_stream: AsyncIterable[Optional[bytes]],
        old_lang_dir: Union[str, Path],
        new_lang_dir: Union[str, Path],
        nbest: int = 1,
        max_fuzzy_cost: Optional[float] = None,
        require_fuzzy: bool = False,
    ) -> List[str]:
        old_lang_dir, new_lang_dir = Path(old_lang_dir), Path(new_lang_dir)
        if self._lat_model is None:
            opts = _lib.default_opts(max_active=self.max_active, lattice_beam=self.lattice_beam, beam=self.beam, acoustic_scale=1.0,
                                     device_id=self.device_id, emit_lattice=1)
            self._lat_model = self._load_model(opts)
        key = str(new_lang_dir)
        if key not in self._rescorers:
            try:
                self._rescorers[key] = _lib.Rescorer(self._lat_model, new_lang_dir)
            except _lib.RsError as e:
                if "No value for disambiguation state" in str(e):
                    raise ValueError("No value for disambiguation state (#0)") from e       # transcribe_stream.py:150-151
                raise
        stream = self._open_stream(self._lat_model)
        loop = asyncio.get_running_loop()
        try:
            async for chunk in audio_stream:
                if chunk:
                    await loop.run_in_executor(None, self._accept_and_advance, stream, chunk)
            try:
                res = await loop.run_in_executor(None, stream.finish, 1, 1.0)
                nbest_stdout = self._rescorers[key].rescore(res, 0, nbest=nbest, acoustic_scale=self.acoustic_scale, key="utt")[0]
            except _lib.RsError as e:
                raise RuntimeError(f"Unexpected error running command online2-cli-nnet3-decode-faster (HIP): {e}") from e
        finally:
            stream.close()
        int2sym_stdout = int2sym(nbest_stdout, read_words_txt(new_lang_dir / "words.txt"))
        _LOGGER.debug("nbest: %s", int2sym_stdout)
        fuzzy_result = get_fuzzy_text(nbest_stdout, old_lang_dir)      # transcribe_stream.py:255-260
        if fuzzy_result is not None:
            text, cost = fuzzy_result
            if cost <= max_fuzzy_cost:
                return [decode_meta(text)]
        if require_fuzzy:
            return []
        return texts_from_int2sym(int2sym_stdout)
