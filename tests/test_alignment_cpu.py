"""Alignments on the host (rs_decode_opts.emit_alignment): the fixtures of tests/golden/alignments.npz
(oracle/gen_alignment_golden.py: the reference's `nbest-to-linear` second output and its `lattice-to-phone-lattice` phone
sequences) held against the reference's own log-likelihoods and costs, the n-best alignment code (lattice.cc) against brute-force
enumeration and the reference's lattices, the phone splitting behind rs_result_phones against the fixtures, and the ABI.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from rhasspy_speech_amd import synth
from tests import cases, endpoint_cases as ec
from tests.lattice_io import nbest as lister_nbest, random_raw_lattice
from tests.test_lattice_cpu import brute_force

ALI = np.load(cases.GOLDEN / "alignments.npz")
INF = float("inf")


def hyps(key: str, what: str):
    """The per-hypothesis lists of record `key` (what: ali / words / phones)."""
    v, off = ALI[f"{key}__{what}"], ALI[f"{key}__{what}_off"]
    return [v[off[k]:off[k + 1]].tolist() for k in range(len(off) - 1)]


def records():
    return sorted({k.rsplit("__", 1)[0] for k in ALI.files if k.endswith("__ali")})


def spec_of(key: str) -> synth.ModelSpec:
    """The model spec behind a fixture record."""
    from tests import length_cases as lc, search_shape_cases as ssc
    kind, name = key.split("__")[:2]
    if kind == "case":
        return cases.case_spec(cases.CASES[name])
    if kind == "shape":
        return ssc.spec()
    if kind == "len":
        return cases.case_spec(lc.case(name))
    return cases.case_spec(cases.CASES[ec.ENDPOINT_CASES[name]["base"]])


def tid_tables(spec: synth.ModelSpec):
    """(phone, hmm state, is self-loop) per transition-id of a synthetic model: two ids per tuple, the self-loop first
    (synth.tid_to_pdf)."""
    tuples = synth.context_tuples(spec)
    phone, state, loop = np.zeros(2 * len(tuples) + 1, np.int32), np.zeros(2 * len(tuples) + 1, np.int32), np.zeros(2 * len(tuples) + 1, bool)
    for k, (p, hs, _f, _s) in enumerate(tuples):
        phone[2 * k + 1] = phone[2 * k + 2] = p
        state[2 * k + 1] = state[2 * k + 2] = hs
        loop[2 * k + 1] = True
    return phone, state, loop


def phones_read_off(spec: synth.ModelSpec, ali):
    """Phone segments of an alignment of a graph built with --reorder=true, from the definition: in such a graph a state's
    self-loops FOLLOW the transition out of it, so a phone is [forward id of its state 0, self-loops, forward id of state 1,
    ...] and a new phone begins exactly at a forward transition-id of HMM state 0 (the ids lattice-to-phone-lattice labels,
    lattice-functions.cc:423-441).  -> [(phone, start, length)], or None where an id does not belong to the phone it follows:
    the padded graphs of tests/search_shape_cases.py have such paths, and SplitToPhones does not split them."""
    phone, state, loop = tid_tables(spec)
    segs = []
    for t, tid in enumerate(ali):
        if not loop[tid] and state[tid] == 0:
            segs.append([int(phone[tid]), t, 0])
        if not segs or segs[-1][0] != phone[tid]:
            return None
        segs[-1][2] += 1
    return [tuple(s) for s in segs]


def phone_starts(spec: synth.ModelSpec, ali):
    """The phones lattice-to-phone-lattice reads off an alignment: one per forward transition-id of HMM state 0."""
    phone, state, loop = tid_tables(spec)
    return [int(phone[t]) for t in ali if not loop[t] and state[t] == 0]


# ---------------------------------------------------------------------------------------------- fixture sanity
def test_fixture_covers_what_it_should():
    from tests import length_cases as lc
    keys = records()
    for name, case in cases.CASES.items():
        for mode in ("offline", "stream"):
            assert f"case__{name}__{mode}" in keys
            n = len(hyps(f"case__{name}__{mode}", "ali"))
            with np.load(cases.GOLDEN / f"{name}.npz") as g:
                n_ref = len(g[f"{mode}_graph_cost"])
            assert n == (min(n_ref, 2) if case.get("big") else n_ref), (name, mode)      # (the big cases keep two hypotheses)
    assert sum(k.startswith("shape__") for k in keys) >= 2 * 5 and sum(k.startswith("ep__") for k in keys) >= 3
    for T in (1, 2, 3):
        for mode in ("offline", "stream"):
            assert [len(a) for a in hyps(f"len__V1__n{lc.samples('V1', T)}__{mode}", "ali")][0] == T


NON_BIG = [n for n, c in cases.CASES.items() if not c.get("big")]


@pytest.mark.parametrize("name", NON_BIG)
def test_fixture_alignments_add_up_to_the_reference_costs(name):
    """sum_t -loglike[t, pdf(tid_t)] = the reference's acoustic cost of the hypothesis, on the reference's own log-likelihoods
    (stored in full for these cases): the fixtures are the reference's alignments, not this library's."""
    id2pdf = synth.tid_to_pdf(cases.case_spec(cases.CASES[name]))
    with np.load(cases.GOLDEN / f"{name}.npz") as g:
        for mode in ("offline", "stream"):
            ll = g[f"{mode}_loglikes"].astype(np.float64)
            alis = hyps(f"case__{name}__{mode}", "ali")
            assert len(alis) == len(g[f"{mode}_acoustic_cost"])
            assert hyps(f"case__{name}__{mode}", "words") == [[int(w) for w in l.split()[1:]] for l in bytes(g[f"{mode}_nbest_text"]).decode().splitlines()]
            for k, a in enumerate(alis):
                assert len(a) == ll.shape[0] == int(g[f"{mode}_num_frames"])
                dev = abs(-ll[np.arange(len(a)), id2pdf[a]].sum() - float(g[f"{mode}_acoustic_cost"][k]))
                print(name, mode, k, "deviation", dev)
                # float accumulation over T frames (the reference sums in float, and prints the cost with 6 digits): the largest
                # deviation over all cases, modes and hypotheses when the fixtures were generated was 2.415e-4; 4 x that
                assert dev < 9.66e-4, (name, mode, k, dev)


@pytest.mark.parametrize("key", records())
def test_fixture_phones_are_the_phones_of_the_fixture_alignments(key):
    spec = spec_of(key)
    for a, ph in zip(hyps(key, "ali"), hyps(key, "phones")):
        assert phone_starts(spec, a) == ph
        segs = phones_read_off(spec, a)
        assert segs is not None or key.startswith("shape__")
        if segs is not None:
            assert [s[0] for s in segs] == ph and sum(s[2] for s in segs) == len(a)


# ---------------------------------------------------------------------------------------------- host n-best alignments
def brute_force_alignments(n_states, final, arcs):
    """{word sequence: (graph, acoustic, transition-ids)} of the best alignment per sequence in CompactLatticeWeight's order:
    total, graph part, shorter string, lexicographic."""
    out = [[] for _ in range(n_states)]
    for a in arcs:
        out[a[0]].append(a)
    best = {}

    def walk(s, words, g, ac, tids):
        if math.isfinite(final[s]):
            key, cand = tuple(words), (g + final[s] + ac, g + final[s], len(tids), list(tids), ac)
            if key not in best or cand[:4] < best[key][:4]:
                best[key] = cand
        for (_, d, w, t, ag, aa) in out[s]:
            walk(d, words + [w] if w else words, g + ag, ac + aa, tids + [t])
    walk(0, [], 0.0, 0.0, [])
    return {k: (v[1], v[4], v[3]) for k, v in best.items()}


@pytest.mark.parametrize("seed", range(24))
def test_nbest_alignments_against_brute_force(seed):
    """Random lattices (tests/test_lattice_cpu.py's); odd seeds put the costs on a 0.5 grid, where alignments tie exactly and the
    string order decides."""
    from rhasspy_speech_amd import _lib
    rng = np.random.default_rng(seed)
    n_states = int(rng.integers(4, 11))
    arcs, final = random_raw_lattice(rng, n_states, fan=3, n_words=3 if seed % 4 < 2 else 2, quantum=0.5 if seed % 2 else 0.0)
    want = brute_force_alignments(n_states, final, arcs)
    if not seed % 2:      # without ties the other test file's enumeration says the same
        assert {k: v[2] for k, v in brute_force(n_states, 0, final, arcs).items()} == {k: v[2] for k, v in want.items()}
    got = _lib.lattice_nbest_alignments_from_raw(n_states, 0, final, arcs, 1e9, 1000)
    assert len(got) == len(want) and len({tuple(w) for w, _, _, _ in got}) == len(got)
    totals = [g + a for _, _, g, a in got]
    assert totals == sorted(totals)
    for words, tids, g, a in got:
        wg, wa, wt = want[tuple(words)]
        assert tids == wt, (words, tids, wt)
        assert g == pytest.approx(wg, abs=1e-5) and a == pytest.approx(wa, abs=1e-5)
    # a beam drops whole hypotheses, never changes an alignment; n cuts the list
    few = _lib.lattice_nbest_alignments_from_raw(n_states, 0, final, arcs, 2.5, 3)
    full = {tuple(h[0]): h[1] for h in got}
    assert 1 <= len(few) <= 3 and few[0][:2] == got[0][:2]
    for words, tids, _, _ in few:
        assert full[tuple(words)] == tids


def raw_of_compact(start, finals, carcs):
    """A CompactLattice as a raw lattice: an arc with k transition-ids becomes a chain of max(k, 1) arcs, the first with the word
    and the costs; a final weight with ids becomes a chain to a new final state."""
    n = len(carcs)
    arcs, final = [], [INF] * n

    def chain(src, dst, label, g, a, tids):
        nonlocal n
        tids = list(tids) or [0]
        for i, t in enumerate(tids):
            d = dst if i == len(tids) - 1 else n
            if d == n:
                n += 1
                final.append(INF)
            arcs.append((src, d, label if i == 0 else 0, t, g if i == 0 else 0.0, a if i == 0 else 0.0))
            src = d
    for s, row in enumerate(carcs):
        for (label, g, a, tids, d) in row:
            chain(s, d, label, g, a, tids)
    for s, (g, a, tids) in finals.items():
        if not tids and a == 0.0:
            final[s] = g
        else:
            end = n
            n += 1
            final.append(0.0)
            chain(s, end, 0, g, a, tids)
    return n, start, final, arcs


def read_decoder_lattice(data: bytes):
    """One table entry as the reference's DECODER writes it -> (start, finals, arcs) in tests/lattice_io.py's form.  (That file's
    reader insists on the header's arc count, which a lattice written by the decoder leaves at 0.)"""
    import struct
    pos = data.index(b" ") + 1

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, data, pos)
        pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def take_str():
        nonlocal pos
        n = take("i")
        pos += n
        return data[pos - n:pos]

    def take_weight():
        g, a = take("ff")
        n = take("i")
        return g, a, [take("i") for _ in range(n)]
    assert take("i") == 2125659606 and take_str() == b"vector" and take_str() == b"compactlattice44"
    take("iiQ")
    start, n_states, _ = take("qqq")
    finals, arcs = {}, []
    for s in range(n_states):
        g, a, tids = take_weight()
        if np.isfinite(g):
            finals[s] = (g, a, tids)
        row = []
        for _ in range(take("q")):
            il, _ol = take("ii")
            g, a, tids = take_weight()
            row.append((il, g, a, tids, take("i")))
        arcs.append(row)
    assert pos == len(data)
    return start, finals, arcs


def reference_lattices():
    import json
    runs = json.loads((cases.GOLDEN / "rescore" / "cases.json").read_text())
    return sorted({r["dir"] for r in runs})


@pytest.mark.parametrize("d", reference_lattices())
def test_nbest_alignments_of_the_reference_decoders_lattices(d):
    """The lattices the reference's decoder wrote (tests/golden/rescore/*/decoder.lat): the five best paths with the alignments
    `lattice-to-nbest | nbest-to-linear` print for them (tests/lattice_io.py's lister, pinned to those tools)."""
    from rhasspy_speech_amd import _lib
    ark = cases.GOLDEN / "rescore" / d / "decoder.lat"
    start, finals, carcs = read_decoder_lattice(ark.read_bytes())
    want = lister_nbest(start, finals, carcs, cases.NBEST)
    assert want and all(len(p["ali"]) == len(want[0]["ali"]) for p in want)
    n, start, final, arcs = raw_of_compact(start, finals, carcs)
    got = _lib.lattice_nbest_alignments_from_raw(n, start, final, arcs, 1e9, cases.NBEST)
    assert [h[0] for h in got] == [p["words"] for p in want]
    assert [h[1] for h in got] == [p["ali"] for p in want]
    for h, p in zip(got, want):
        assert h[2] == pytest.approx(p["graph"], abs=2e-3) and h[3] == pytest.approx(p["acoustic"], abs=2e-3)


# ---------------------------------------------------------------------------------------------- phone splitting
@pytest.fixture(scope="module")
def mdl_of(tmp_path_factory):
    """final.mdl of a fixture record's model, written once per distinct spec."""
    built = {}

    def get(key):
        spec = spec_of(key)
        k = repr(spec)
        if k not in built:
            root = tmp_path_factory.mktemp("mdl")
            synth.write_model_dir(root / "model", spec)
            built[k] = root / "model" / "model" / "model" / "final.mdl"
        return built[k]
    return get


@pytest.mark.parametrize("key", records())
def test_phone_splitting_reproduces_the_fixture_phones(mdl_of, key):
    """rs_result_phones' splitting (through the host entry rs_alignment_phones, on the model's own final.mdl)."""
    from rhasspy_speech_amd import _lib
    spec = spec_of(key)
    phone_of, _, _ = tid_tables(spec)
    for a, want in zip(hyps(key, "ali"), hyps(key, "phones")):
        if phones_read_off(spec, a) is None or not _ends_a_phone(spec, a):
            with pytest.raises(_lib.RsError, match=r"Could not split word into phones correctly \(forced-out\?\)") as ei:
                _lib.alignment_phones(mdl_of(key), a)
            assert ei.value.status == _lib.RS_ERR_DECODE
            continue
        ph, start, length = _lib.alignment_phones(mdl_of(key), a)
        assert ph.tolist() == want
        assert int(length.sum()) == len(a) and start.tolist() == [0] + np.cumsum(length)[:-1].tolist() and (length > 0).all()
        for p, s, l in zip(ph, start, length):
            assert (phone_of[a[s:s + l]] == p).all()
        assert list(zip(ph.tolist(), start.tolist(), length.tolist())) == phones_read_off(spec, a)


def _ends_a_phone(spec, ali) -> bool:
    """Whether the alignment's last phone reached its last HMM state (a finalize at an endpoint may stop inside a phone)."""
    _, state, _ = tid_tables(spec)
    last = spec.hmm_states - 1 if not spec.chain_topology else 0
    return state[ali[-1]] == last


def test_an_alignment_that_does_not_split_is_refused(mdl_of):
    from rhasspy_speech_amd import _lib
    key = "case__tiny_hmm_u6__offline"
    a = hyps(key, "ali")[0]
    phone, _, loop = tid_tables(spec_of(key))
    other = next(t for t in range(1, len(phone)) if loop[t] and phone[t] != phone[a[0]])
    # a self-loop that belongs to another phone than the transition it follows, in the middle and at the end
    for bad in (a[:1] + [other] + a[1:], a + [other], [other]):
        with pytest.raises(_lib.RsError, match="Could not split word into phones correctly") as ei:
            _lib.alignment_phones(mdl_of(key), bad)
        assert ei.value.status == _lib.RS_ERR_DECODE
    with pytest.raises(_lib.RsError, match="no transition-id of the model"):
        _lib.alignment_phones(mdl_of(key), [1, 10 ** 6])
    ph, start, length = _lib.alignment_phones(mdl_of(key), [])
    assert len(ph) == len(start) == len(length) == 0


# ---------------------------------------------------------------------------------------------- ABI
def test_abi():
    from rhasspy_speech_amd import _lib
    lib = _lib.lib()
    assert C.sizeof(_lib.DecodeOpts) == 72                                 # what it was before the option took reserved[0]
    assert _lib.DecodeOpts.emit_alignment.offset == 64 and _lib.DecodeOpts.stream_min_ticks.offset == 60
    assert _lib.DecodeOpts.reserved.offset == 68 and _lib.DecodeOpts.emit_lattice.offset == 44
    for sym in ("rs_result_alignment", "rs_result_alignment_text", "rs_result_phones", "rs_lattice_nbest_alignments_from_raw", "rs_alignment_phones"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    assert _lib.default_opts().emit_alignment == 0
    # a null result is a bad argument, not a crash
    ids, n = C.POINTER(C.c_int32)(), C.c_int32()
    assert lib.rs_result_alignment(None, 0, 0, C.byref(ids), C.byref(n)) == _lib.RS_ERR_ARG
    assert lib.rs_result_alignment_text(None, 0, b"utt", None, 0) == _lib.RS_ERR_ARG
    assert lib.rs_result_phones(None, 0, 0, C.byref(ids), C.byref(ids), C.byref(ids), C.byref(n)) == _lib.RS_ERR_ARG


def test_unset_is_not_a_value_of_the_option(case_cache):
    from rhasspy_speech_amd import _lib
    model_dir, graph_dir, _, _ = case_cache("tiny_u0")
    for bad in (_lib.RS_OPT_UNSET, 2):
        with pytest.raises(_lib.RsError, match="rs_decode_opts.emit_alignment must be 0 or 1"):
            _lib.Model(model_dir, graph_dir, _lib.default_opts(emit_alignment=bad))
    _lib.Model(model_dir, graph_dir, _lib.default_opts(emit_alignment=1))      # host-side parse only
