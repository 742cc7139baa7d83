"""The arenas of a decode call (rhasspy_speech_amd/csrc/arena.h) without a GPU: tests/host/arena_check.cc instantiates Arena over
malloc / free backends that record their calls and poison what they free, is built once with the host compiler under the address
and undefined-behaviour sanitizers and run as a child process.  The program asserts alignment, the reserved tail of a block and that
the buffers of a round stay intact and apart (also across a spill into further blocks); what it prints -- the backend's calls and
where every pointer lies -- is checked here against what arena.h promises."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
MIB = 1 << 20
KINDS = {"dev": (256, MIB), "host": (64, 0)}      # alignment, reserved tail of a block


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("arena") / "arena_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "arena_check.cc"), "-o", str(exe)], check=True)

    def run(kind, rounds):
        """Per round of requests on one fresh arena: (allocations, frees, synchronisations, blocks, bytes, [(block, offset)]).  The
        sanitizers must stay silent, and the arena's destruction must free every block once (the program checks)."""
        cmds = [f"new {kind}"] + ["round " + " ".join(map(str, r)) for r in rounds]
        p = subprocess.run([str(exe)], input="".join(c + "\n" for c in cmds), capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
        lines = p.stdout.splitlines()
        assert len(lines) == len(cmds) and lines[0] == "new"
        out = []
        for line in lines[1:]:
            head, _, where = line[len("round "):].partition("|")
            out.append(tuple(int(x) for x in head.split()) + ([tuple(int(v) for v in w.split(":")) for w in where.split()],))
        return out
    return run


def one_block_offsets(req, align):
    at, out = 0, []
    for r in req:
        at = -(-at // align) * align
        out.append((0, at))
        at += r
    return out, at


def random_requests(rng, total):
    """Requests that add up to about `total` bytes: many small ones, a few large, some empty, odd sizes."""
    req = []
    while sum(req) < total:
        kind = rng.random()
        if kind < 0.1:
            req.append(0)
        elif kind < 0.7:
            req.append(int(rng.integers(1, 4097)))
        else:
            req.append(int(rng.integers(1, max(total // 3, 2))))
    return req


@pytest.mark.parametrize("kind", list(KINDS))
def test_spill_then_one_block_for_good(check, kind):
    align, _tail = KINDS[kind]
    rng = np.random.default_rng(11)
    req = [0, 1, 255, 0, 3 * MIB + 17, 64, 5 * MIB + 1, 0, 12345, 9 * MIB, 7]
    rounds = [req] * 4 + [req[:5], [1], []] + [req] * 2 + [random_requests(rng, 6 * MIB)]
    out = check(kind, rounds)
    want, total = one_block_offsets(req, align)
    # the cold round: several blocks, and (the program has checked) every buffer of it intact at the end
    assert out[0][3] > 1 and out[0][1] == 0 and out[0][2] == 0
    # the Reset after it: one synchronisation, every block freed, one block for the whole round; then nothing moves, round after round
    for k in (1, 2, 3):
        assert out[k][:4] == (out[0][0] + 1, out[0][0], 1, 1), k
        assert out[k][4] >= total + total // 8 + MIB and out[k][5] == want, k
    # smaller rounds, then the large one again, then another of no more bytes: no backend call, the same offsets
    for k in range(4, 10):
        assert out[k][:5] == out[1][:5], k
        assert out[k][5] == one_block_offsets(rounds[k], align)[0], k


@pytest.mark.parametrize("kind", list(KINDS))
def test_cold_rounds_make_few_allocations(check, kind):
    """A round of N bytes from an empty arena: at most ceil(log2 N) + 2 backend allocations; the round after it has one block."""
    align, _tail = KINDS[kind]
    rng = np.random.default_rng(5)
    totals = [1, 300, MIB - 1, MIB + 1, 3 * MIB] + [int(2 ** e) for e in rng.uniform(10, 25, 12)]
    for total in totals:
        req = random_requests(rng, total)
        if total == 3 * MIB:
            req = [256] * (3 * MIB // 256)       # (nothing but small requests: every block is left full)
        cold, warm, again = check(kind, [req, req, req])
        n = one_block_offsets(req, align)[1]
        assert cold[0] <= math.ceil(math.log2(max(n, 1))) + 2, (total, cold[:5])
        assert warm[3] == 1 and warm[0] == cold[0] + (1 if cold[3] > 1 else 0)
        assert again[:5] == warm[:5] and again[5] == warm[5] == one_block_offsets(req, align)[0]


def test_growing_rounds(check):
    """Every new largest round spills once and is coalesced by the next Reset; a round that fits allocates nothing."""
    sizes = [100, 2 * MIB, 2 * MIB, 2 * MIB, 5 * MIB, 300, 5 * MIB, 5 * MIB + 4 * MIB // 8, 40 * MIB, 40 * MIB, 1]
    out = check("dev", [[s // 2, s - s // 2] for s in sizes])
    allocations = [o[0] for o in out]
    # 100 B: the first block; 2 MiB: a second block, then one for both; 5 MiB: again; 5.5 MiB: inside the eighth of headroom;
    # 40 MiB: a block per half (the first is sized for what the round has asked for so far)
    assert allocations == [1, 2, 3, 3, 4, 5, 5, 5, 7, 8, 8]
    assert [o[3] for o in out] == [1, 2, 1, 1, 2, 1, 1, 1, 3, 1, 1]
    assert [o[2] for o in out] == [0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3]      # a synchronisation only with a coalescing Reset
