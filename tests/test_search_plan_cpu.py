"""The host-only policy of the search (rhasspy_speech_amd/csrc/search_plan.{h,cc}) without a GPU:
tests/host/search_plan_check.cc is built once with the host compiler under the address and undefined-behaviour sanitizers and
run as a child process.  Every line it prints -- a graph, a request kind, the batch size, the longest utterance, the CU count, the
RS_* switches, then the search, its kernel instantiation, grid and LDS bytes, the lattice route and the capacities planned for it --
is compared with tests/host/search_plan_expected.txt, a recording of the code as it was before the policy moved into one module
(how it was made: the head of search_plan_check.cc).  A few decisions are also worked out here by hand from the comments of
search_plan.cc, so that the recording is held to the intent.  The program itself asserts that the planned LDS bytes cover every
region of the kernels' shared carve-up, stay within a CU's 160 KB, and that the token capacity fits an int or the plan says so."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
EXPECTED = ROOT / "tests" / "host" / "search_plan_expected.txt"


@pytest.fixture(scope="module")
def decisions(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("search_plan") / "search_plan_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "search_plan_check.cc"), str(CSRC / "search_plan.cc"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    return p.stdout.splitlines()


def test_every_decision_is_the_recorded_one(decisions):
    want = EXPECTED.read_text().splitlines()
    assert EXPECTED.stat().st_size < 200 * 1024
    assert len(decisions) == len(want) > 800
    for got, exp in zip(decisions, want):
        assert got == exp


def _decision(lines, case):
    """The line for `case` ('<graph> <request> n<n_utts> T<maxT> cu<CUs> <switches>') as a dict: 'search' (reg, reg-exact, dense,
    live, tokens), 'kernel' ('RegDecode<512,4,2>'), 'lattice' (none, dense-rows, rows-to-tokens, tokens), 'lattice_kernel', 'windows',
    and every name=value field as an int (the lattice kernel's with the prefix 'lattice_')."""
    hits = [l for l in lines if l.startswith(case + " | ")]
    assert len(hits) == 1, case
    parts = hits[0].split(" | ")[1:]
    search, kernel, *rest = parts[0].split()
    d = dict(search=search, kernel=kernel, windows="windows" in rest)
    d.update({k: int(v) for k, v in (f.split("=") for f in rest if "=" in f)})
    route, *lat = parts[1].split()
    d["lattice"] = route.split("=")[1]
    d["lattice_kernel"] = lat[0] if lat else None
    d.update({"lattice_" + k: int(v) for k, v in (f.split("=") for f in lat[1:])})
    for f in parts[2].split():
        k, v = f.split("=")
        d[k] = v if k == "opts" else int(v)
    return d


def test_hand_derived_anchors(decisions):
    """grammar625: 625 states, 1800 emitting and 600 epsilon arcs -- they fit <512,4,2> (2048 / 1024 arcs) --, epsilon depth 1, at most
    12 + 4 arcs per state, so the exact-order kernel applies.  256 CUs unless the case says otherwise."""
    for lines in (decisions, EXPECTED.read_text().splitlines()):
        # (the sweep runs the switch sets with 4 utterances, the plain cases with 1 unless the batch size is what is swept)
        case = lambda request, n=None, sw="-", graph="grammar625", cu=256: _decision(
            lines, f"{graph} {request} n{n or (1 if sw == '-' else 4)} T298 cu{cu} {sw}")
        # the crowded rule: 4 n_utts >= 3 CUs -> 192 of 256 CUs; half the waves, twice the arcs per thread
        d = case("best", 191)
        assert (d["search"], d["kernel"], d["grid"], d["threads"]) == ("reg", "RegDecode<512,4,2>", 191, 512)
        d = case("best", 192)
        assert (d["search"], d["kernel"], d["grid"], d["threads"]) == ("reg", "RegDecode<256,8,4>", 192, 256)
        # 304 CUs: 228 utterances
        assert case("best", 227, cu=304)["kernel"] == "RegDecode<512,4,2>" and case("best", 228, cu=304)["kernel"] == "RegDecode<256,8,4>"
        # a stream window never gets the crowded shape; one in which no stream ends stages nothing: cost_cur (626 floats, rounded up
        # to 16 bytes: 2512) + 626 keys of 8 bytes
        for n in (192, 512):
            d = case("window", n)
            assert (d["kernel"], d["windows"], d["stage"], d["lds"]) == ("RegDecode<512,4,2>", True, 0, 2512 + 626 * 8)
            d = case("finish", n)
            assert (d["kernel"], d["windows"], d["stage"], d["lds"]) == ("RegDecode<512,4,2>", True, 32 * 1024, 32 * 1024)
        # a whole-utterance batch launch stages 32 KB for the traceback, a time slab that ends no utterance nothing
        assert case("best", 191)["stage"] == 32 * 1024 and case("best", 191)["lds"] == 32 * 1024
        assert _decision(lines, "grammar625 slab n1 T298 cu256 -")["stage"] == 0
        # cap_pf = min(max(4 max_active, 8192), S); an n-best call on a grammar graph keeps every state of every frame
        assert _decision(lines, "grammar625 best n1 T298 cu256 -")["cap_pf"] == 625
        assert _decision(lines, "big_s100000 best n1 T298 cu256 -")["cap_pf"] == 28000
        assert _decision(lines, "big_s100000 active1000 n1 T298 cu256 -")["cap_pf"] == 8192
        d = _decision(lines, "grammar625 nbest5_per_frame500 n1 T298 cu256 -")
        assert (d["cap_pf"], d["tok_cap"]) == (625, 300 * 625)
        assert _decision(lines, "grammar625 per_frame500 n1 T298 cu256 -")["cap_pf"] == 500
        # RS_DECODER
        assert (case("best", sw="DECODER=sparse")["search"], case("nbest5", sw="DECODER=sparse")["search"]) == ("tokens", "tokens")
        assert case("best", sw="DECODER=hash")["search"] == "live"
        assert (case("best", sw="DECODER=dense")["search"], case("best", sw="DECODER=dense")["kernel"]) == ("dense", "DenseDecode<256,1>")
        d = case("nbest5", sw="DECODER=dense")
        assert (d["search"], d["lattice"]) == ("live", "tokens")
        # the n-best call of a grammar graph: the register-resident search, the lattice on its rows; 2400 arcs on 512 threads are 5
        # per thread, the rung above is 6; 24 bytes of rows per state + 16
        d = case("nbest5")
        assert (d["search"], d["kernel"], d["lattice"], d["lattice_kernel"]) == ("reg", "RegDecode<512,4,2>", "dense-rows", "DenseLattice<512,6>")
        assert (d["lattice_lds"], d["lattice_eps_rounds"]) == (625 * 24 + 16, 1)
        # each switch moves the one enum it names
        t = case("nbest5", sw="LATTICE_SEARCH=tokens")
        assert (t["search"], t["lattice"]) == ("live", "tokens")
        t = case("nbest5", sw="LATTICE_KERNEL=tokens")
        assert (t["search"], t["kernel"], t["lattice"]) == ("reg", d["kernel"], "rows-to-tokens")
        t = case("nbest5", sw="LATTICE_KERNEL=vote")
        assert (t["search"], t["lattice"], t["lattice_kernel"], t["lattice_eps_rounds"]) == ("reg", "dense-rows", d["lattice_kernel"], -1)
        for sw in ("LATTICE_SEARCH=tokens", "LATTICE_KERNEL=tokens", "LATTICE_KERNEL=vote"):
            assert case("best", sw=sw) == dict(case("best"), grid=4)
        # exact_token_order: the exact kernel where the graph allows it, and then no register-resident n-best; 33 arcs of a state
        # do not fit the kernel's 32-bit mask
        for request, sw in (("exact", "-"), ("best", "EXACT_ORDER=1")):
            d = case(request, sw=sw)
            assert (d["search"], d["kernel"], d["opts"]) == ("reg-exact", "RegDecodeExact<512,4,2>", "1,0")
        assert case("exact", sw="EXACT_ORDER=0")["search"] == "reg"
        d = case("exact_nbest5")
        assert (d["search"], d["lattice"]) == ("live", "tokens")
        d = case("exact", graph="exact_e33")
        assert (d["search"], d["kernel"], d["opts"]) == ("reg", "RegDecode<512,4,2>", "1,0")
        assert case("exact_nbest5", graph="exact_e33")["lattice"] == "dense-rows"
        assert case("best", sw="REG_NO_HIST=1")["opts"] == "0,1"
        # graphs the LDS-resident searches cannot hold: the live table, unless its records cannot name the arcs
        assert _decision(lines, "arpa best n1 T298 cu256 -")["search"] == "live"
        assert _decision(lines, "arcs_2p30m1 best n1 T298 cu256 -")["search"] == "live"
        assert _decision(lines, "arcs_2p30 best n1 T298 cu256 -")["search"] == "tokens"
        # (76693 + 2) x 28000 tokens still fit an int (2^31 / 28000 = 76695.8), one frame more does not
        assert [l for l in lines if l.startswith("arpa best n4 T76694 ")][0].endswith("| error=decoder token capacity overflows; lower max_tokens_per_frame")
        assert _decision(lines, "arpa best n4 T76693 cu256 -")["tok_cap"] == 76695 * 28000
