"""`bench.py --dump-outputs DIR`: the last timed step's results as .npy files, so that two builds can be compared output for
output.  The record decoding runs on any host; the end-to-end run needs the GPU (`-m gpu`)."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench

ROOT = Path(__file__).resolve().parent.parent


def _cost_bits(g, a):
    return list(np.array([g, a], np.float32).view(np.int32))


def test_dump_of_packed_records(tmp_path):
    """rs_result_pack records {status, n_words, 62 ids, graph / acoustic cost bits}; a failed utterance keeps no words."""
    rec = np.zeros((3, 66), np.int32)
    rec[0, :4] = [0, 2, 17, 5]
    rec[0, -2:] = _cost_bits(1.5, -20.25)
    rec[1, :2] = [-3, 0]
    rec[2, :3] = [0, 1, 9]
    rec[2, -2:] = _cost_bits(0.5, 7.0)
    bench.dump_outputs(tmp_path, None, rec, sharded=False)
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == {"status", "n_words", "words", "graph_cost", "acoustic_cost"}
    np.testing.assert_array_equal(got["status"], [0, -3, 0])
    np.testing.assert_array_equal(got["n_words"], [2, 0, 1])
    np.testing.assert_array_equal(got["words"], [[17, 5], [-1, -1], [9, -1]])
    np.testing.assert_array_equal(got["graph_cost"], np.float32([1.5, 0.0, 0.5]))
    np.testing.assert_array_equal(got["acoustic_cost"], np.float32([-20.25, 0.0, 7.0]))
    for name, a in got.items():
        assert a.dtype == (np.float32 if name.endswith("cost") else np.float64), name


def test_dump_of_sharded_records_is_in_utterance_order(tmp_path):
    """rs_decode_batch_sharded records {utterance, status, n_words, 63 ids, cost bits}, gathered rank by rank: stored by utterance."""
    rec = np.zeros((4, 68), np.int32)
    for row, utt in enumerate([0, 2, 1, 3]):          # two ranks' rows, utterance i on rank i % 2
        rec[row, :4] = [utt, 0, 1, 100 + utt]
        rec[row, -2:] = _cost_bits(utt, -utt)
    bench.dump_outputs(tmp_path, None, rec, sharded=True)
    np.testing.assert_array_equal(np.load(tmp_path / "words.npy"), [[100], [101], [102], [103]])
    np.testing.assert_array_equal(np.load(tmp_path / "graph_cost.npy"), np.float32([0, 1, 2, 3]))
    np.testing.assert_array_equal(np.load(tmp_path / "acoustic_cost.npy"), np.float32([0, -1, -2, -3]))


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """The headline workload with a few timed steps: the line reports exactly those steps and, without --full, nothing beside
    them; the dumped transcripts are the reference's (tests/golden/configs/c1_grammar)."""
    from tests import configs
    out = tmp_path / "out"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] == pytest.approx(1000.0 * line["timed_seconds"] / 3)
    assert not set(line) & {"roofline", "stages_ms", "cpu_baseline", "other_workloads", "steady_state", "hbm_resident", "nbest5", "tdnnf_model"}
    ref_words, _, _ = configs.load_golden("c1_grammar")
    words = np.load(out / "words.npy")
    assert words.shape[0] == len(ref_words) == 256
    assert [[int(w) for w in row if w >= 0] for row in words] == ref_words
    np.testing.assert_array_equal(np.load(out / "status.npy"), np.zeros(256))
    assert np.load(out / "graph_cost.npy").dtype == np.float32 and np.load(out / "num_frames.npy").min() > 0
