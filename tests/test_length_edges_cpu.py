"""CPU test that PINS the oracle at the utterance-length edges (tests/length_cases.py): Oracle.transcribe and
Oracle.transcribe_stream on every length of every variant against what the reference's binaries gave (tests/golden/lengths/*.npz,
oracle/gen_length_golden.py), at the tolerances of tests/test_oracle_golden.py.  Runs without a GPU."""
import numpy as np
import pytest

from tests import length_cases as lc
from tests.test_oracle_golden import parse_nbest

NBEST = 5


def check_offline(orc, g, n, clip):
    k = lc.key(n)
    if int(g[f"{k}_offline_status"]) != 0:
        with pytest.raises(RuntimeError) as ei:
            orc.transcribe(clip, nbest=NBEST)
        assert str(ei.value) == lc.reference_error(g, n, "offline")
        return
    tr = orc.transcribe(clip, nbest=NBEST)
    assert tr.num_frames == int(g[f"{k}_offline_num_frames"])
    assert tr.feats.shape == g[f"{k}_input"].shape
    fd = np.abs(tr.feats - g[f"{k}_input"])
    assert fd.max() < 2e-4 and np.quantile(fd, 0.99) < 1e-4, ("features", fd.max(), np.quantile(fd, 0.99))
    if f"{k}_offline_ivector" in g:
        d = np.abs(tr.ivector - g[f"{k}_offline_ivector"][0]).max()
        assert d < 1e-4, ("iVector", d)
    rows = lc.stored_rows(g, n, "offline", tr.num_frames)
    assert tr.loglikes[rows].shape == g[f"{k}_offline_loglikes"].shape
    d = np.abs(tr.loglikes[rows] - g[f"{k}_offline_loglikes"]).max()
    assert d < 1e-4, ("log-likelihoods", d)
    ref = parse_nbest(bytes(g[f"{k}_offline_nbest_text"]))
    got = [p.words for p in tr.nbest]
    assert got == ref, (got, ref)
    np.testing.assert_allclose([p.graph_cost for p in tr.nbest], g[f"{k}_offline_graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose([p.acoustic_cost for p in tr.nbest], g[f"{k}_offline_acoustic_cost"], rtol=2e-4, atol=2e-3)
    assert tr.text().split() == bytes(g[f"{k}_offline_nbest_text"]).split()


def check_stream(orc, g, n, clip):
    k = lc.key(n)
    if int(g[f"{k}_stream_status"]) != 0:
        with pytest.raises(RuntimeError) as ei:
            orc.transcribe_stream(clip, nbest=NBEST)
        assert str(ei.value) == lc.reference_error(g, n, "stream")
        return
    sched, _L, _R = orc.stream_schedule(len(clip))
    if f"{k}_stream_chunk_tick" in g:
        assert [j for j, _ in sched] == [int(x) for x in g[f"{k}_stream_chunk_tick"]]
    tr = orc.transcribe_stream(clip, nbest=NBEST)
    assert tr.num_frames == int(g[f"{k}_stream_num_frames"])
    if f"{k}_stream_ivector" in g:
        assert tr.ivector.shape == g[f"{k}_stream_ivector"].shape
        d = np.abs(tr.ivector - g[f"{k}_stream_ivector"]).max()
        assert d < 1e-4, ("iVectors", d)
    rows = lc.stored_rows(g, n, "stream", tr.num_frames)
    assert tr.loglikes[rows].shape == g[f"{k}_stream_loglikes"].shape
    d = np.abs(tr.loglikes[rows] - g[f"{k}_stream_loglikes"]).max()
    assert d < 1e-4, ("log-likelihoods", d)
    assert [p.words for p in tr.nbest] == parse_nbest(bytes(g[f"{k}_stream_nbest_text"]))
    np.testing.assert_allclose([p.graph_cost for p in tr.nbest], g[f"{k}_stream_graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose([p.acoustic_cost for p in tr.nbest], g[f"{k}_stream_acoustic_cost"], rtol=2e-4, atol=2e-3)
    assert tr.text() == bytes(g[f"{k}_stream_nbest_text"])


@pytest.mark.parametrize("variant", list(lc.VARIANTS))
def test_oracle_matches_reference_at_every_length(tmp_path, variant):
    """Every length of the variant, offline and streamed; every failing one is reported."""
    from oracle import pipeline
    g = lc.load_golden(variant)
    ns = list(lc.lengths(variant))
    assert [int(x) for x in g["lengths"]] == ns                      # the golden file is the table's
    model_dir, graph_dir, pcm = lc.build_variant_files(variant, tmp_path)
    orc = pipeline.Oracle(model_dir, graph_dir, **lc.VARIANTS[variant].get("opts", {}))
    bad = []
    for n in ns:
        for mode, check in (("offline", check_offline), ("stream", check_stream)):
            try:
                check(orc, g, n, pcm[:n])
            except Exception as e:                                   # noqa: BLE001 (whatever the oracle raises at an edge is a finding)
                bad.append(f"{variant} n={n} ({lc.num_frames(variant, n)} frames) {mode}: {type(e).__name__}: {str(e).strip()[:300]}")
    assert not bad, "\n".join([f"{len(bad)} of {2 * len(ns)} failed"] + bad)


def test_length_table_covers_what_it_names():
    """The table itself: counts per variant, every variant's clips without a frame, and every frame-counted entry (classes A, B, E,
    V8's list) giving the number of frames it is named for -- with j extra samples too, and one sample less giving one frame less."""
    # (4720 samples is both a tick edge and 28 frames; with the 1600-sample window 5120 samples is 23 frames)
    want = {"V1": 44, "V2": 37, "V3": 44, "V4": 37, "V5": 37, "V6": 37, "V7": 38, "V8": 10}
    no_frame = {v: {0, 1, 399} for v in want}
    no_frame["V7"] = {0, 1, 400, 1599, 1023, 1024, 1025}      # (the tick edges below the 1600-sample window)
    no_frame["V8"] = {399}
    for v, cnt in want.items():
        ls = lc.lengths(v)
        assert len(ls) == cnt, (v, len(ls))
        assert {n for n in ls if lc.num_frames(v, n) == 0} == no_frame[v], v
        assert all("D" in ls[n] for n in no_frame[v] if n not in lc.CLASS_C), v
        classes = lc.VARIANTS[v]["classes"]
        named = ([(T, j, "A") for T, j in lc.CLASS_A] if "A" in classes else []) + ([(T, 0, "B") for T in lc.CLASS_B] if "B" in classes else []) + \
                ([(T, 0, "E") for T in lc.CLASS_E] if "E" in classes else []) + ([(T, 0, "A" if T <= 12 else "B") for T in lc.V8_FRAMES] if "8" in classes else [])
        for T, j, cls in named:
            n = lc.samples(v, T, j)
            assert cls in ls[n] and lc.num_frames(v, n) == T and lc.num_frames(v, n - j - 1) == T - 1, (v, T, j)
            assert n <= lc.FULL, (v, T)
    assert lc.lengths("V7")[400] == "D" and lc.lengths("V7")[1599] == "D" and lc.num_frames("V7", 1600) == 1
    assert lc.num_frames("V1", lc.samples("V1", 1, 159)) == 1 and lc.num_frames("V1", lc.samples("V1", 1, 160)) == 2
