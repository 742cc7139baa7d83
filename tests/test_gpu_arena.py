"""The arenas of a decode call grow on demand (rhasspy_speech_amd/csrc/arena.h): calls of changing shape on one model -- the cold
call that spills into further blocks, the call after it that coalesces them, the warm calls -- give bit for bit what the same call
gives on a freshly loaded model, and the `arenas:` line of rs_model_describe stands still once the model has seen its largest
call twice.  Tiny models only: the shapes are the smallest that reach every allocation path (batch: register-resident, token-list
with the live-state tables, decoder-row gather, no extractor, each with and without the lattice buffers; streams: advance, partial,
endpoint, adaptation, finalize)."""
import re

import pytest

from rhasspy_speech_amd import _lib
from tests import cases

pytestmark = pytest.mark.gpu

TICK = 1024


def arenas(model):
    """{'device': (blocks, bytes, allocations), 'host': ...} of the model's `arenas:` line."""
    m = re.search(r"^arenas: device blocks=(\d+) bytes=(\d+) allocations=(\d+); host blocks=(\d+) bytes=(\d+) allocations=(\d+)$", model.describe(), re.M)
    assert m, model.describe()
    v = [int(x) for x in m.groups()]
    return {"device": tuple(v[:3]), "host": tuple(v[3:])}


def utt_record(res, u, lattice=False):
    """Everything a call returns for utterance u (or its error), exact: float costs as they are."""
    try:
        rec = [res.num_frames(u), [(res.words(u, k), res.costs(u, k)) for k in range(res.num_hyps(u))]]
        if lattice:
            rec.append(res.lattice(u))
        return rec
    except _lib.RsError as e:
        return ["error", str(e)]


def batches():
    u3 = cases.case_audio(cases.CASES["tiny_u3_short"])
    u0 = cases.case_audio(cases.CASES["tiny_u0"])
    assert len(u3) == 9000
    # mixed lengths: nothing at all, exactly one frame (a 400-sample window), one sample short of / beyond a tick, odd counts
    eight = [u0, u0[:0], u0[:400], u3, u0[:20000], u0[5000:36001], u3[:4097], u0[1000:32999]]
    return [u3], eight


@pytest.mark.parametrize("name,emit_lattice", [("tiny_u0", 0), ("tiny_u0", 1), ("tiny_arpa_u7", 0), ("tiny_arpa_u7", 1), ("tiny_fsf3_u16", 0),
                                               ("tiny_noiv_u2", 0)])
def test_batch_calls_of_changing_shape(case_cache, name, emit_lattice):
    md, gd, _wav, _pcm = case_cache(name)
    opts = lambda: _lib.default_opts(emit_lattice=emit_lattice)
    single, eight = batches()

    def call(model, pcms, nbest):
        res = model.decode_batch(pcms, nbest=nbest)
        return [utt_record(res, u, lattice=bool(emit_lattice)) for u in range(len(pcms))]

    fresh = {(len(p), nbest): call(_lib.Model(md, gd, opts()), p, nbest) for p in (single, eight) for nbest in (1, 5)}
    assert fresh[8, 5][0][0] != "error" and len(fresh[8, 5][0][1]) >= 1 and fresh[8, 1][0][1][0][0]      # (the long utterance says something)
    model = _lib.Model(md, gd, opts())
    for nbest in (1, 5):
        for k, pcms in enumerate((single, eight, single, eight)):
            assert call(model, pcms, nbest) == fresh[len(pcms), nbest], (nbest, k)
        after_second = arenas(model)
        # one context, one utterance group: one device and one host arena in use, each coalesced into one block
        assert after_second["device"][0] == 1 and after_second["host"][0] == 1, after_second
        assert call(model, eight, nbest) == fresh[8, nbest]
        third = arenas(model)
        assert third == after_second, (nbest, after_second, third)
    print(name, emit_lattice, arenas(model))


def stream_run(model, pcms):
    """The streams fed tick by tick in batched calls, a partial and an endpoint query on every tick (a stream takes part while it
    has samples left), then finalize and the adaptation export.  Per stream: [per-tick records, final record, adaptation state]."""
    ep = _lib.default_endpoint_opts("1")
    streams = [_lib.Stream(model) for _ in pcms]
    recs = [[] for _ in pcms]
    for t in range(max((len(p) + TICK - 1) // TICK for p in pcms)):
        live = [i for i, p in enumerate(pcms) if len(p) > t * TICK]
        batch = [streams[i] for i in live]
        _lib.accept_streams(batch, [pcms[i][t * TICK:(t + 1) * TICK] for i in live])
        part = _lib.partial_streams(batch)
        ends = _lib.endpoint_streams(batch, ep)
        for j, i in enumerate(live):
            recs[i].append((utt_record(part, j), ends[j].as_tuple()))
    fin = _lib.finalize_streams(streams, nbest=1)
    states = _lib.adaptation_of_streams(streams)
    out = [[recs[i], utt_record(fin, i), {k: v.tobytes() for k, v in states[i].arrays().items()}] for i in range(len(pcms))]
    for s in streams:
        s.close()
    return out


def test_stream_calls_of_changing_shape(case_cache):
    """Every run makes 24 advances (23 full ticks of its longest stream and the finalize), a multiple of every depth the rotation
    over the arena sets can be built with (2, 3, 4): the runs meet the sets the same way, so the repeat of the eight-stream run is
    the steady state of every set."""
    md, gd, _wav, _pcm = case_cache("tiny_u0")
    u0 = cases.case_audio(cases.CASES["tiny_u0"])
    lengths = [23 * TICK, TICK, 5000, 9000, 16 * TICK, 12345, 20000, 3000]
    pcms = [u0[7 * i:7 * i + n] for i, n in enumerate(lengths)]
    alone = [stream_run(_lib.Model(md, gd, _lib.default_opts()), [p])[0] for p in pcms]
    assert len(alone[0][0]) == 23 and alone[0][1][0] != "error" and alone[0][1][1][0][0], alone[0][1]      # (the long stream says something)
    model = _lib.Model(md, gd, _lib.default_opts())
    assert stream_run(model, pcms[:1]) == alone[:1]
    assert stream_run(model, pcms) == alone
    assert stream_run(model, pcms[:1]) == alone[:1]
    before = arenas(model)
    assert stream_run(model, pcms) == alone
    after = arenas(model)
    assert after == before, (before, after)
    print("streams", after)
