"""The host-only launch policy of the layer GEMM (rhasspy_speech_amd/csrc/gemm_launch.{h,cc}) without a GPU:
tests/host/gemm_launch_check.cc is built once with the host compiler under the address and undefined-behaviour sanitizers and
run as a child process.  Every line it prints -- a layer, a row count, share / exclusive, the RS_GEMM_* switches, then the kernel
instantiation and the grid planned for it -- is compared with tests/host/gemm_launch_expected.txt, a recording of the launch code
as it was before the policy moved into one module (how it was made: the head of gemm_launch_check.cc).  A few decisions are also
worked out here by hand from the comments of gemm_launch.cc and nnet_gemm_b3j.hip, so that the recording is held to the intent.
The program itself asserts that the planned grid, decoded the way the kernels decode blockIdx, owns every (row, column tile)
exactly once."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
EXPECTED = ROOT / "tests" / "host" / "gemm_launch_expected.txt"


@pytest.fixture(scope="module")
def decisions(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("gemm_launch") / "gemm_launch_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "gemm_launch_check.cc"), str(CSRC / "gemm_launch.cc"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    return p.stdout.splitlines()


def test_every_decision_is_the_recorded_one(decisions):
    want = EXPECTED.read_text().splitlines()
    assert EXPECTED.stat().st_size < 200 * 1024
    assert len(decisions) == len(want) > 1000
    for got, exp in zip(decisions, want):
        assert got == exp


def _decision(lines, case):
    """{'kernel': 'B3J<...>', 'blocks': ..., 'nbig': ..., ...} of the line for `case` ('<layer> <rows> s<share> x<excl> <switches>')."""
    hits = [l for l in lines if l.startswith(case + " | ")]
    assert len(hits) == 1, case
    kernel, *fields = hits[0].split(" | ")[1].split()
    return dict(kernel=kernel, **{k: int(v) for k, v in (f.split("=") for f in fields)})


def test_hand_derived_anchors(decisions):
    """256 CUs, share 1: 512 slots of two workgroups per CU.  The hidden layer is image-fed, strip-eligible, 48 k-steps, one column
    tile.  Kernel names are B3J<WM,MIXED,STRIP,SDIV,MRT,WN>, B3I<MR,MIXED,KPS>, Exact<MT,WM,WN,vec,dma>."""
    for lines in (decisions, EXPECTED.read_text().splitlines()):
        # 640 tiles of 128 rows are two rounds of the 512 slots, 512 tiles of 160 rows are one, and K is long: the 160-row tile
        d = _decision(lines, "hidden 81920 s1 x0 -")
        assert (d["kernel"], d["nbig"], d["blocks"], d["threads"], d["res"]) == ("B3J<1,0,1,2,5,4>", 512, 512, 256, 0)
        # 513 tiles of 160 rows no longer fit one round: one whole round of 128-row tiles, the 16 385 rows behind them as 257 tiles of
        # 64 rows, 256 of them (half the slots) in front; three ranges padded to multiples of 8
        d = _decision(lines, "hidden 81921 s1 x0 -")
        assert (d["kernel"], d["nbig"], d["nfirst"], d["blocks"]) == ("B3J<1,1,1,2,4,4>", 512, 256, 512 + 256 + 8)
        # a stream advance: less than one round of 32-row tiles -> 128 of them on GemmKernelB3J, which adds a residual itself
        for layer in ("hidden", "res"):
            d = _decision(lines, f"{layer} 4096 s1 x0 -")
            assert (d["kernel"], d["nbig"], d["blocks"], d["res"], d["img"]) == ("B3J<1,1,0,4,4,4>", 0, 128, 0, 1)
            d = _decision(lines, f"{layer} 4096 s1 x0 B3J_SMALL=0")
            assert (d["kernel"], d["nbig"], d["blocks"], d["res"]) == ("B3I<1,0,8>", 128, 128, int(layer == "res"))
        # the threshold: 512 slots x 32 rows still go as 32-row tiles, one row more is GemmKernelB3J's own launch (no whole round of
        # 128-row tiles: 257 tiles of 64 rows, 256 in front)
        assert _decision(lines, "hidden 16384 s1 x0 -")["kernel"] == "B3J<1,1,0,4,4,4>"
        d = _decision(lines, "hidden 16385 s1 x0 -")
        assert (d["kernel"], d["nbig"], d["nfirst"], d["blocks"]) == ("B3J<1,1,1,2,4,4>", 0, 256, 256 + 8)
        # 128 columns: the 256 x 128 tile, 320 of them in one round
        d = _decision(lines, "bottleneck128 81920 s1 x0 -")
        assert (d["kernel"], d["nbig"], d["blocks"]) == ("B3J<2,0,0,2,4,2>", 320, 320)
        # 40 columns, no split weights: exact FP32 with aligned sources (DMA form), four waves stacked on one 64-column tile, no
        # image.  1280 tiles of 64 rows are 5 rounds of the 256 CUs (5 x 64 x 0.97), 640 of 128 rows are 3 (3 x 128): 64 rows
        d = _decision(lines, "lda40 81920 s1 x0 -")
        assert (d["kernel"], d["nbig"], d["blocks"], d["img"], d["res"]) == ("Exact<1,4,1,1,1>", 1280, 1280, 0, 0)
        # RS_GEMM_B3=0: everything on the exact kernels, no operand images
        for layer in ("hidden", "output362", "res"):
            d = _decision(lines, f"{layer} 81920 s1 x0 B3=0")
            assert d["kernel"].startswith("Exact<") and d["img"] == 0 and d["res"] == 0
