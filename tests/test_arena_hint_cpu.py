"""Reset(stream, expect) of the decode arenas (rhasspy_speech_amd/csrc/arena.h) and the mark that sibling decode contexts share,
without a GPU: tests/host/arena_hint_check.cc is built with the host compiler -- under the address and undefined-behaviour
sanitizers for the single-arena cases, under the thread sanitizer for the shared mark -- and run as a child process.  The program
asserts alignment, the reserved tail, that buffers stay intact and apart and that every block is freed exactly once; what it prints
-- the backend's calls, the round's size and where every pointer lies -- is checked here against what arena.h promises: a cold arena
that is told the round of a warm sibling makes one allocation and never coalesces, and a hint is never needed to be right."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MIB = 1 << 20
KINDS = {"dev": (256, MIB), "host": (64, 0)}      # alignment, reserved tail of a block
REQ = [0, 1, 255, 0, 3 * MIB + 17, 64, 5 * MIB + 1, 0, 12345, 9 * MIB, 7]      # (tests/test_arena_cpu.py: test_spill_then_one_block_for_good)


def compile_check(tmp_path_factory, name, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", *sanitize, "-pthread", str(ROOT / "tests" / "host" / "arena_hint_check.cc"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = compile_check(tmp_path_factory, "arena_hint_check", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])

    def run(kind, rounds):
        """`rounds`: (expect or None for the plain Reset, requests), on one fresh arena.  Per round: (allocations, frees,
        synchronisations, blocks, bytes, round, [(block, offset)]).  The sanitizers must stay silent, and the arena's destruction
        must free every block once (the program checks)."""
        cmds = [f"new {kind}"] + [" ".join(["round" if e is None else f"hint {e}"] + [str(x) for x in r]) for e, r in rounds]
        p = subprocess.run([str(exe)], input="".join(c + "\n" for c in cmds), capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
        lines = p.stdout.splitlines()
        assert len(lines) == len(cmds) and lines[0] == "new"
        out = []
        for line in lines[1:]:
            head, _, where = line.split(" ", 1)[1].partition("|")
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


def block_rule(need, tail):
    return need + need // 8 + MIB + tail


@pytest.mark.parametrize("kind", list(KINDS))
def test_no_hint_is_the_plain_reset(check, kind):
    lists = [REQ] * 4 + [REQ[:5], [1], []] + [REQ] * 2 + [[4 * MIB, 2 * MIB + 3]]
    plain = check(kind, [(None, r) for r in lists])
    assert check(kind, [(0, r) for r in lists]) == plain
    assert plain[0][3] > 1 and plain[1][:4] == (plain[0][0] + 1, plain[0][0], 1, 1)      # (the lists do spill and coalesce)


@pytest.mark.parametrize("kind", list(KINDS))
def test_cold_arena_told_its_siblings_round(check, kind):
    align, _tail = KINDS[kind]
    want, total = one_block_offsets(REQ, align)
    sibling = check(kind, [(None, REQ)])[0]
    assert sibling[3] > 1 and sibling[5] == total
    out = check(kind, [(sibling[5], REQ)] * 4)
    for k, o in enumerate(out):      # the cold round and three repeats: one allocation in all, nothing freed, nothing waited for
        assert o[:4] == (1, 0, 0, 1), (k, o[:6])
        assert o[4] >= total + total // 8 + MIB and o[5] == total and o[6] == want, (k, o[:6])


@pytest.mark.parametrize("kind", list(KINDS))
def test_round_larger_than_the_hint(check, kind):
    align, _tail = KINDS[kind]
    want, total = one_block_offsets(REQ, align)
    cold, second, third, fourth = check(kind, [(total // 2, REQ)] * 4)
    assert cold[3] > 1 and cold[1] == 0 and cold[2] == 0 and cold[5] == total      # it spills ...
    assert second[:4] == (cold[0] + 1, cold[0], 1, 1)                              # ... and is coalesced with one synchronisation
    assert second[4] >= total + total // 8 + MIB and second[6] == want
    assert third == second and fourth == second                                    # one block, and nothing moves


@pytest.mark.parametrize("kind", list(KINDS))
def test_coalescing_for_a_larger_hint(check, kind):
    align, tail = KINDS[kind]
    expect = 40 * MIB + 12345
    large = [expect // 2 // align * align, expect - expect // 2 // align * align]      # a round of exactly `expect` bytes
    assert one_block_offsets(large, align)[1] == expect
    cold, coalesced, big, again = check(kind, [(None, REQ), (expect, REQ), (0, large), (None, REQ)])
    assert cold[3] > 1
    assert coalesced[:4] == (cold[0] + 1, cold[0], 1, 1) and coalesced[4] >= block_rule(expect, tail) and coalesced[6] == one_block_offsets(REQ, align)[0]
    assert big[:5] == coalesced[:5] and big[5] == expect and big[6] == one_block_offsets(large, align)[0]
    assert again[:5] == coalesced[:5]


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_block_is_left_alone(check, kind):
    first, at_reset, small, grown, after = check(kind, [(None, [100]), (50 * MIB, []), (50 * MIB, [100, 7]), (50 * MIB, [3 * MIB]), (50 * MIB, [3 * MIB])])
    assert first[:4] == (1, 0, 0, 1)
    assert at_reset[:5] == first[:5] and small[:5] == first[:5]      # a sibling's larger call: no backend call at Reset, none after it
    # its own round outgrows the block: a spill, then one block for what the sibling saw
    assert grown[:4] == (2, 0, 0, 2)
    assert after[:4] == (3, 2, 1, 1) and after[4] >= block_rule(50 * MIB, KINDS[kind][1])


def test_shared_mark_under_the_thread_sanitizer(tmp_path_factory):
    exe = compile_check(tmp_path_factory, "arena_hint_check_tsan", ["-fsanitize=thread"])
    p = subprocess.run([str(exe), "marks", "4", "300"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    fields = dict(f.split("=") for f in p.stdout.split()[1:])
    assert fields["threads"] == "4" and fields["rounds"] == "300"
    assert 1 <= int(fields["unhinted"]) <= 4 and int(fields["unhinted"]) + int(fields["hinted"]) == 1200
