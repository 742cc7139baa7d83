"""The host-only call planning (rhasspy_speech_amd/csrc/call_plan.{h,cc}) without a GPU: tests/host/call_plan_check.cc is built
once with the host compiler under the address and undefined-behaviour sanitizers and run as a child process; what it prints is
compared with the CPU restatements (oracle/pipeline.py: stream_schedule and the iVector-row provider of loglikes_stream;
tests/endpoint_cases.py: frames_after_ticks) and with values this file works out from the comments of call_plan.h.  The program
itself asserts that every index array of a stream advance stays inside the stream's rows."""
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from oracle.pipeline import Oracle
from tests import endpoint_cases, length_cases as lc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
TICK = 1024
K_MAX_LISTS = 24          # kernels.h: BatchSetup::kMaxLists

# name: window, shift, chunk, L, R (halo), Rm (the network's right context), extractor, splice left / right, subsampling factor
CONFIGS = {
    "zamia": dict(window=400, shift=160, chunk=24, L=15, R=15, Rm=15, has_iv=1, sl=3, sr=3, fsf=1),
    "fsf3": dict(window=400, shift=160, chunk=21, L=6, R=6, Rm=6, has_iv=1, sl=3, sr=3, fsf=3),
    "chunk30": dict(window=400, shift=160, chunk=30, L=4, R=4, Rm=4, has_iv=1, sl=3, sr=3, fsf=1),
    "noiv": dict(window=400, shift=160, chunk=24, L=4, R=4, Rm=4, has_iv=0, sl=0, sr=0, fsf=1),
    "win1600": dict(window=1600, shift=160, chunk=24, L=4, R=4, Rm=4, has_iv=1, sl=3, sr=3, fsf=1),
}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("call_plan") / "call_plan_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "call_plan_check.cc"), str(CSRC / "call_plan.cc"), "-o", str(exe)], check=True)

    def run(cfg, commands):
        """Output lines (without the command word) of `commands` under configuration `cfg`; the sanitizers must stay silent."""
        c = CONFIGS[cfg]
        head = "cfg {window} {shift} {chunk} {L} {R} {Rm} {has_iv} {sl} {sr} {fsf}\n".format(**c)
        p = subprocess.run([str(exe)], input=head + "".join(x + "\n" for x in commands), capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
        lines = p.stdout.splitlines()
        assert len(lines) == len(commands) + 1
        return [l.split(" ", 1)[1] if " " in l else "" for l in lines[1:]]
    return run


def stub(cfg):
    """What stream_schedule, stream_ivector_rows and frames_after_ticks read of an Oracle."""
    c = CONFIGS[cfg]
    mfcc = SimpleNamespace(num_frames=lambda n: 0 if n < c["window"] else 1 + (n - c["window"]) // c["shift"])
    nnet = SimpleNamespace(context=lambda: (c["L"], c["Rm"]), halo=max(c["L"], c["R"]))
    return SimpleNamespace(mfcc=mfcc, nnet=nnet, chunk=c["chunk"], fsf=c["fsf"], ie={"right": c["sr"]} if c["has_iv"] else None)


def ints(s):
    return [int(x) for x in s.split()]


def sample_counts(cfg):
    w = CONFIGS[cfg]["window"]
    ns = set(range(0, 3 * TICK + 401))
    for m in range(TICK, 30 * 16000 + 1, TICK):
        ns.update(m + d for d in (0, 1, -1, 160, -160, 400, -400))
    frames = list(range(1, 13)) + list(range(23, 32)) + [47, 48, 49, 199, 200, 201, 599, 600, 601, 602]
    ns.update(w + 160 * (T - 1) for T in frames)
    for v in lc.VARIANTS:
        ns.update(lc.lengths(v))
    return sorted(ns)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_flushed_schedule_is_the_oracles(check, cfg):
    orc, ns = stub(cfg), sample_counts(cfg)
    out = check(cfg, [f"sched {n}" for n in ns])
    for n, line in zip(ns, out):
        assert ints(line) == [last for _, last in Oracle.stream_schedule(orc, n)[0]], n


def _chunks_of(groups):
    """stream output -> per advance (ticks, chunks scheduled, decoder frames, t0, t1, [(chunk, last)], n_riv)."""
    adv = []
    for g in groups.split("|"):
        head, _, riv = g.partition("/")
        v = ints(head)
        adv.append((v[0], v[1], v[2], v[3], v[4], list(zip(v[5::2], v[6::2])), ints(riv)))
    return adv


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_resumed_schedule_equals_the_one_shot_schedule(check, cfg):
    """However the samples are split into deliveries, the chunks scheduled are those of the flushed one-shot schedule; without the
    flush the decoder frames after every tick are those of frames_after_ticks."""
    orc, c = stub(cfg), CONFIGS[cfg]
    rng = np.random.default_rng(24)
    cap = -(-max(4096, 2 * c["chunk"]) // c["chunk"]) * c["chunk"]
    totals = [0, 399, 5000, 5120, 97000, 480000] + [int(x) for x in rng.integers(1, 480001, 10)]
    cmds, want = [], []
    for total in totals:
        splits = [[total], sorted(set(int(x) for x in rng.integers(0, total + 1, int(rng.integers(1, 40)))) | {total})]
        if total >= 5000:
            splits.append(list(range(1, 5001)) + ([total] if total > 5000 else []))
        for s in splits:
            cmds.append(f"stream 1 0 {cap} " + " ".join(map(str, s)))
            want.append(total)
    for total, line in zip(want, check(cfg, cmds)):
        adv = _chunks_of(line)
        got = [ch for a in adv for ch in a[5]]
        ref = [last for _, last in Oracle.stream_schedule(orc, total)[0]]
        assert got == list(enumerate(ref)), total
        assert adv[-1][0] == (total + TICK - 1) // TICK and adv[-1][4] == orc.mfcc.num_frames(total)
    # no flush: one advance per tick
    totals = [t for t in totals if t >= TICK][:8]
    out = check(cfg, [f"stream 0 0 {cap} " + " ".join(str(TICK * (j + 1)) for j in range(t // TICK)) for t in totals])
    for total, line in zip(totals, out):
        adv = _chunks_of(line)
        assert [a[2] for a in adv] == endpoint_cases.frames_after_ticks(orc, total), total
        assert [a[0] for a in adv] == list(range(1, total // TICK + 1))


def replaced_loop(T, nch, L, R, chunk, Rm, base):
    """The per-row loop of DecodeGroup that FillIvecRows replaces."""
    out = []
    for r in range(T + L + R):
        k = 0
        if nch > 0:
            slot = ((r - L) // chunk) * chunk
            while k < nch - 1 and slot >= (k + 1) * chunk + Rm:
                k += 1
        out.append(base + k)
    return out


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if CONFIGS[c]["has_iv"]])
def test_ivector_row_map(check, cfg):
    orc, c = stub(cfg), CONFIGS[cfg]
    L, R, chunk = c["L"], c["R"], c["chunk"]
    rng = np.random.default_rng(7)
    ns = [0, 399, c["window"], 5120, 97000, 48000] + [lc.samples("V1", T) for T in (23, 24, 25, 47, 48, 49)] + [int(x) for x in rng.integers(0, 200000, 12)]
    out = check(cfg, ["batch " + " ".join(map(str, ns))])[0].split("|")
    max_chunks, base, row_ivec = ints(out[0])[0], ints(out[1]), ints(out[2])
    fb, fe, orow, act = (np.array(ints(x)).reshape(max_chunks, len(ns)) for x in out[3:7])
    at = 0
    for u, n in enumerate(ns):
        T = orc.mfcc.num_frames(n)
        sched = [last for _, last in Oracle.stream_schedule(orc, n)[0]]
        nch = len(sched)
        assert base[u + 1] - base[u] == max(nch, 1)
        got = row_ivec[at:at + T + L + R]
        at += T + L + R
        assert got == replaced_loop(T, nch, L, R, chunk, c["Rm"], base[u]), n
        if nch:
            assert got == [base[u] + int(k) for k in Oracle.stream_ivector_rows(orc, nch, np.arange(-L, T + R))], n
        # the estimator's steps: what loglikes_stream does chunk by chunk
        done = 0
        for k in range(max_chunks):
            if k < nch and sched[k] + 1 > done:
                assert (fb[k, u], fe[k, u], act[k, u]) == (done, sched[k] + 1, 1)
                done = sched[k] + 1
            else:
                assert act[k, u] == 0
            assert orow[k, u] == (base[u] + k if k < nch else -1)
    assert at == len(row_ivec) and max_chunks == max(1, max(len(Oracle.stream_schedule(orc, n)[0]) for n in ns))
    # a stream advance: the rows [t0 - L, t1 + R) read what the map says, at most the last chunk scheduled so far
    total = 97000
    cap = -(-4096 // chunk) * chunk
    deliveries = sorted(set(int(x) for x in rng.integers(0, total, 25)) | {total})
    nch = len(Oracle.stream_schedule(orc, total)[0])
    for ticks, sched_n, _dec, t0, t1, _chunks, riv in _chunks_of(check(cfg, [f"stream 1 1 {cap} " + " ".join(map(str, deliveries))])[0]):
        want = [] if t1 <= t0 else [min(int(k), max(sched_n - 1, 0)) for k in Oracle.stream_ivector_rows(orc, nch, np.arange(t0 - L, t1 + R))]
        assert riv == want, (t0, t1)


def brute_span(runs, w):
    rows = np.concatenate([np.arange(f, f + e) for f, e in runs]) if runs else np.zeros(0, int)
    if len(rows) == 0:
        return 0
    if len(rows) < w:
        return int(rows[-1] - rows[0] + 1)
    return int((rows[w - 1:] - rows[:len(rows) - w + 1]).max() + 1)


def runs_of(T, L, R, lext, rext):
    base = np.concatenate([[0], np.cumsum(np.asarray(T) + L + R)])
    return [(int(base[u]) + L - lext, int(t) + lext + rext) for u, t in enumerate(T) if t > 0]


def short_run_batch():
    """The frames of test_gpu_length_edges.py's _short_run_batch: 320 clips, most of one to three frames, runs of up to three
    clips without a frame in between."""
    rng = np.random.default_rng(8)
    T = []
    while len(T) < 320:
        r = rng.random()
        if r < 0.72:
            T.append((1, 2, 3)[int(rng.integers(0, 3))])
        elif r < 0.80:
            T.extend([0] * int(rng.integers(1, 4)))
        elif r < 0.96:
            T.append((5, 8, 12, 24, 25)[int(rng.integers(0, 5))])
        else:
            T.append(29)
    return T[:320]


def test_span_of_runs_bounds_every_window(check, capsys):
    rng = np.random.default_rng(3)
    batches = [short_run_batch(), [1] * 512, [300, 0, 0, 0, 300], [0, 0, 1, 0, 0], [1], []]
    for p in ([0.1, 0.3, 0.15, 0.15, 0.25, 0.05], [0.4, 0.3, 0.1, 0.1, 0.05, 0.05]):      # seeded mixes of run lengths 0, 1, 2, 3, 29, 300
        for _ in range(12):
            batches.append([int(t) for t in rng.choice([0, 1, 2, 3, 29, 300], int(rng.integers(2, 260)), p=p)])
    T0 = np.array(batches[0])
    assert ((T0 >= 1) & (T0 <= 3)).sum() >= 200 and (T0 == 0).sum() >= 20
    cases = []
    for T in batches:
        for L, R in ((15, 15), (6, 6)):
            for lext, rext in ((0, 0), (L - 1, R - 1), (3, 3), (L - 3, 0)):
                for w in (128, 160):
                    cases.append((runs_of(T, L, R, lext, rext), w))
    out = check("zamia", [f"span {w} " + " ".join(f"{f} {e}" for f, e in runs) for runs, w in cases])
    loose = 0
    for (runs, w), line in zip(cases, out):
        got, brute = int(line), brute_span(runs, w)
        assert got >= brute, (runs, w, got, brute)
        if got > brute:
            loose += 1
            print(f"SpanOfRuns({len(runs)} runs, {w}) = {got}: {got - brute} rows above the widest window")
    print(f"{loose} of {len(cases)} bounds are loose")


def chain_net(layer_offsets, f):
    """(L, R, [(lext, rext, stride) of every layer's output]) of a chain of layers that read their input at the given offsets:
    a layer's output keeps as much halo as the layers after it reach, and is evaluated at t = 0 mod f only when nothing reads
    it elsewhere (the output is read at t = 0 mod f)."""
    n = len(layer_offsets)
    lext, rext, res = [0] * (n + 1), [0] * (n + 1), [None] * n + [{0}]
    for i in reversed(range(n)):
        lext[i] = lext[i + 1] + max(0, -min(layer_offsets[i]))
        rext[i] = rext[i + 1] + max(0, max(layer_offsets[i]))
        res[i] = {(r + o) % f for r in res[i + 1] for o in layer_offsets[i]}
    return lext[0], rext[0], [(lext[i + 1], rext[i + 1], f if f > 1 and res[i + 1] == {0} else 1) for i in range(n)]


def expected_lists(T, L, R, ops, n_slabs, trim=True):
    """The row lists call_plan.h describes: the frames in slab-major order; then the strided buffers' lists (rows t = 0 mod stride
    of [-lext, T + rext)); then, all or nothing, the trimmed halos (t in [-lext, T + rext)) while there is room."""
    n, maxT = len(T), max(T, default=0)
    if sum(T) == 0:
        return 0, []
    slab_len = max(1, -(-maxT // n_slabs))
    segs, acc = [], 0
    for k in range(n_slabs):
        for t in T:
            segs.append(acc)
            acc += min(max(t - k * slab_len, 0), slab_len)
    lists = [dict(lext=0, rext=0, stride=1, first=0, n_segs=n_slabs * n, total=sum(T), L_eff=L, slab_len=slab_len, segs=segs + [acc])]
    needs = []
    for lext, rext, st in ops:
        if lext > L or rext > R or (st == 1 and ((lext, rext) == (0, 0) or (lext >= L and rext >= R))):
            continue
        if (lext, rext, st) not in needs:
            needs.append((lext, rext, st))
    if len(needs) + 1 > K_MAX_LISTS:
        trim = False
    for strided in (True, False):
        for lext, rext, st in needs:
            if (st > 1) != strided or (st == 1 and not trim):
                continue
            if len(lists) >= K_MAX_LISTS:
                if st > 1:
                    return 2, []
                continue
            per = [0 if t == 0 else (t + lext + rext if st == 1 else (t + rext - 1) // st + lext // st + 1) for t in T]
            lists.append(dict(lext=lext, rext=rext, stride=st, first=lext % st, n_segs=n, total=sum(per), L_eff=L - lext,
                              slab_len=max(maxT + lext + rext, 1), segs=[0] + [int(x) for x in np.cumsum(per)]))
    return 0, lists


ZAMIA = ((-1, 0, 1), (0,), (-1, 0, 1), (-1, 0, 1), (-3, 0, 3), (-3, 0, 3), (-3, 0, 3), (-3, 0, 3), (0,), (0,))
TINY_FSF3 = ((-1, 0, 1), (0,), (-1, 0, 1), (-1, 0, 1), (-3, 0, 3), (0,), (0,))
# (the factorised net: every layer a linear bottleneck without context, then the affine part with the offsets)
TINYF = ((-1, 0, 1), (0,), (0,), (0,), (-1, 0, 1), (0,), (-1, 0, 1), (0,), (-3, 0, 3), (0,), (0,))


@pytest.mark.parametrize("name,offsets,f,n_slabs", [
    ("zamia", ZAMIA, 1, 1), ("zamia, three slabs", ZAMIA, 1, 3), ("zamia, every third frame", ZAMIA, 3, 1), ("factorised", TINYF, 1, 1),
    ("f = 3, L = R = 6", TINY_FSF3, 3, 1), ("30 extents", ((-1, 0, 1),) * 30, 1, 1), ("30 strided extents", ((-3, 0, 3),) * 30, 3, 1)])
def test_row_list_plan(check, name, offsets, f, n_slabs):
    L, R, ops = chain_net(offsets, f)
    if name == "zamia":
        assert (L, R) == (15, 15) and ops[0][:2] == (14, 14) and ops[-1][:2] == (0, 0)      # (15 rows a side for the first, none for the last)
    if name == "f = 3, L = R = 6":
        assert (L, R) == (6, 6) and [o[2] for o in ops] == [1, 1, 1, 3, 3, 3, 3]
    for T in (short_run_batch()[:60], [0, 0, 0], [300, 1, 0, 29, 64, 0, 0, 2], [97]):
        for trim in (1, 0):
            status, want = expected_lists(T, L, R, ops, n_slabs, bool(trim))
            cmd = f"lists {n_slabs} {K_MAX_LISTS} {trim} {L} {R} {len(T)} " + " ".join(map(str, T)) + f" {len(ops)} " + " ".join(f"{a} {b} {c}" for a, b, c in ops)
            parts = check("zamia", [cmd])[0].split("|")
            assert ints(parts[0]) == [status], (name, T, parts[0])
            if status:
                continue
            got = []
            for p in parts[2:]:
                head, _, segs = p.partition(":")
                v = ints(head)
                got.append(dict(lext=v[0], rext=v[1], stride=v[2], first=v[3], n_segs=v[4], total=v[5], L_eff=v[6], slab_len=v[7], segs=ints(segs)))
                if v[2] == 1 and (n_slabs == 1 or len(got) > 1):      # spans: a bound for the list it describes (one slab: in utterance order)
                    runs = runs_of(T, L, R, v[0], v[1])
                    assert v[8] >= brute_span(runs, 128) and v[9] >= brute_span(runs, 160)
                else:
                    assert v[8] == 0 and v[9] == 0
            assert got == want, (name, T, trim)
            if want:
                assert ints(parts[1]) == [want[0]["segs"][k * len(T)] for k in range(n_slabs)] + [want[0]["total"]]
    if name == "30 extents":
        assert len(expected_lists([5, 5], L, R, ops, 1)[1]) == 1          # more lists than a call carries: full halos everywhere
    if name == "30 strided extents":
        assert expected_lists([5, 5], L, R, ops, 1)[0] == 2
