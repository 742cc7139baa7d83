"""The walk the recurrent block kernels share (csrc/recurrent_walk.h: which rows a chain visits, where a stream advance re-enters,
which step's state row is parked) without a GPU: a stand-alone host program under the address and undefined-behaviour sanitizers."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_chain_set_up_against_an_enumeration_under_sanitizers(tmp_path):
    """tests/host/recurrent_walk_check.cc (its own main) calls RecChainSetUp for every chain index of the grid -- delays 1 to 8, every
    stride that divides the delay, left / right / re-entry extents 0 to delay + 1, lengths 0 to 2 delay + 3, batch calls and stream
    advances at t0 = 0, 1, delay, delay + 1, two utterances of different lengths and slots -- and compares with rows it enumerates
    from the definition: every row of a chain's class visited exactly once, empty and absent utterances without steps, the
    continuation flag, the parked step and the ring row of every chain, no ring row shared."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "recurrent_walk_check"
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "recurrent_walk_check.cc"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("recurrent walk: ") and lines[0].endswith(" all as enumerated"), p.stdout
    assert int(lines[0].split()[2]) > 100000      # (the sweep ran: 8 delays x strides x 3 extents x lengths x 5 call kinds)
