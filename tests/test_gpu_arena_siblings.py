"""A decode context that serves its first call sizes its arenas from what its siblings have seen (rhasspy_speech_amd/csrc/engine.h:
Model's round marks; arena.h: Reset(stream, expect)): once one context of a model is warm, every further context makes ONE backend
allocation per arena for its first call -- no spill into further blocks, no coalescing call after it -- and returns bit for bit
what a freshly loaded model returns.  Tiny model, 24 mixed-length utterances in one utterance group; the further contexts come into
use through three calls started together from three threads."""
import threading

import pytest

from rhasspy_speech_amd import _lib
from tests.test_gpu_arena import arenas, batches, utt_record

pytestmark = pytest.mark.gpu


def test_further_contexts_take_one_allocation_each(case_cache):
    md, gd, _wav, _pcm = case_cache("tiny_u0")
    pcms = batches()[1] * 3

    def call(model):
        res = model.decode_batch(pcms, nbest=1)
        return [utt_record(res, u) for u in range(len(pcms))]

    fresh = call(_lib.Model(md, gd, _lib.default_opts()))
    assert fresh[0][0] != "error" and fresh[0][1][0][0], fresh[0]      # (the long utterance says something)
    model = _lib.Model(md, gd, _lib.default_opts())
    assert call(model) == fresh and call(model) == fresh
    alone = arenas(model)
    assert alone["device"][0] == 1 and alone["host"][0] == 1, alone
    d0, h0 = alone["device"][2], alone["host"][2]

    def concurrent_round():
        barrier = threading.Barrier(3)
        out = [None] * 3

        def body(i):
            try:
                barrier.wait()
                out[i] = call(model)
            except BaseException as e:      # (reported by the assertion below, on the main thread)
                out[i] = e
        threads = [threading.Thread(target=body, args=(i,)) for i in range(3)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for i, rec in enumerate(out):
            assert rec == fresh, (i, rec if isinstance(rec, BaseException) else "records differ from the fresh model's")
        return arenas(model)

    n, seen = 1, None
    for k in range(5):
        seen = concurrent_round()
        n = seen["device"][0]
        print("round", k, seen)
        assert n >= 1 and seen["host"][0] == n, seen
        assert seen["device"][2] == d0 + (n - 1) and seen["host"][2] == h0 + (n - 1), (k, alone, seen)
        if n >= 2:
            break
    assert n >= 2, f"the calls of five rounds of three threads never overlapped: only one decode context was ever used ({seen})"
    after = concurrent_round()
    assert after == seen, (seen, after)
