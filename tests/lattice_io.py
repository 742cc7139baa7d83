"""Test helpers for the lattice wire format: a reader of binary CompactLattice table entries written from the format's
description (kaldi-lattice.cc:478-500, OpenFst VectorFst layout), and a lister of a lattice's n best paths that prints what the
REFERENCE's `lattice-to-nbest --n=N --acoustic-scale=1.0 | nbest-to-linear` prints for it.  The lister is pinned to those tools'
own output by tests/golden/lattice_tools.json (oracle/gen_lattice_tools_golden.py; tests/test_lattice_cpu.py)."""
import heapq
import itertools
import struct
from pathlib import Path

import numpy as np


def read_compact_lattice(entry: bytes, key: str):
    """Parser of one binary table entry: returns (start, finals{state: (g, a, tids)}, arcs[state] = [(label, g, a, tids, dst)])."""
    head = key.encode() + b" "
    assert entry.startswith(head)
    start, finals, arcs, pos = _read_fst(entry, len(head))
    assert pos == len(entry)
    return start, finals, arcs


def read_compact_lattice_table(data: bytes):
    """Every entry of a binary table (entries back to back, as an `ark:` file holds them): [(key, start, finals, arcs)]."""
    out, pos = [], 0
    while pos < len(data):
        sp = data.index(b" ", pos)
        start, finals, arcs, end = _read_fst(data, sp + 1)
        out.append((data[pos:sp].decode(), start, finals, arcs))
        pos = end
    return out


def _read_fst(entry: bytes, pos: int):
    def take(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, entry, pos)
        pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def take_str():
        nonlocal pos
        n = take("i")
        s = entry[pos:pos + n]
        pos += n
        return s

    def take_weight():
        g, a = take("ff")
        n = take("i")
        tids = list(take(f"{n}i")) if n > 1 else ([take("i")] if n == 1 else [])
        return g, a, tids

    assert take("i") == 2125659606                       # OpenFst magic
    assert take_str() == b"vector"
    assert take_str() == b"compactlattice44"
    version, flags = take("ii")
    assert version == 2 and flags == 0
    take("Q")
    start, n_states, n_arcs = take("qqq")
    finals, arcs, seen = {}, [], 0
    for s in range(n_states):
        g, a, tids = take_weight()
        if np.isfinite(g):
            finals[s] = (g, a, tids)
        row = []
        for _ in range(take("q")):
            il, ol = take("ii")
            assert il == ol                              # acceptor
            g, a, tids = take_weight()
            row.append((il, g, a, tids, take("i")))
        seen += len(row)
        arcs.append(row)
    assert seen == n_arcs
    return start, finals, arcs, pos


def random_raw_lattice(rng, n_states, fan, n_words, eps_rate=0.3, quantum=0.0):
    """Acyclic state-level lattice in time order: arcs go forward, a share of them carry no word (label 0).  quantum > 0
    rounds the costs to multiples of it, which makes equal-cost alignments common."""
    def cost(scale):
        c = rng.random() * scale
        return float(np.float32(round(c / quantum) * quantum if quantum else c))
    arcs = []
    tid = 1
    for s in range(n_states - 1):
        for _ in range(int(rng.integers(1, fan + 1))):
            d = int(rng.integers(s + 1, min(n_states, s + 4)))
            w = 0 if rng.random() < eps_rate else int(rng.integers(1, n_words + 1))
            arcs.append((s, d, w, tid, cost(3), cost(5)))
            tid += 1
    final = [float("inf")] * n_states
    final[n_states - 1] = cost(1)
    if n_states > 3:
        final[n_states - 2] = cost(2)
    return arcs, final


def nbest(start, finals, arcs, n: int):
    """The n best paths of an acyclic CompactLattice, best first under LatticeWeight's order (total cost, then graph cost:
    fstext/lattice-weight.h:294-307) -- the paths lattice-to-nbest extracts, with nbest-to-linear's fields: words, alignment
    (the transition-ids of the arcs and of the final weight, in order), graph cost, acoustic cost.  A* over the lattice with the
    exact best completion of every state as its estimate, so complete paths leave the queue in order."""
    inf = (float("inf"), float("inf"))
    best = [None] * len(arcs)                                  # best (total, graph) from a state to the end
    stack = [(start, False)]
    while stack:                                               # iterative post-order: lattices are long chains of states
        s, done = stack.pop()
        if best[s] is not None:
            continue
        if not done:
            stack.append((s, True))
            stack.extend((a[4], False) for a in arcs[s] if best[a[4]] is None)
            continue
        b = (finals[s][0] + finals[s][1], finals[s][0]) if s in finals else inf
        for (_, g, a, _, d) in arcs[s]:
            b = min(b, (g + a + best[d][0], g + best[d][1]))
        best[s] = b
    out, tie = [], itertools.count()
    if best[start] == inf:
        return out
    queue = [(best[start], next(tie), start, 0.0, 0.0, (), ())]
    while queue and len(out) < n:
        _, _, s, g, a, words, ali = heapq.heappop(queue)
        if s is None:
            out.append(dict(words=list(words), ali=list(ali), graph=g, acoustic=a))
            continue
        if s in finals:
            fg, fa, ft = finals[s]
            heapq.heappush(queue, ((g + fg + a + fa, g + fg), next(tie), None, g + fg, a + fa, words, ali + tuple(ft)))
        for (label, ag, aa, at, d) in arcs[s]:
            if best[d] != inf:
                g2, a2 = g + ag, a + aa
                heapq.heappush(queue, ((g2 + a2 + best[d][0], g2 + best[d][1]), next(tie), d, g2, a2,
                                       words + (label,) if label else words, ali + tuple(at)))
    return out


def reference_paths(ark: Path, n: int):
    """`lattice-to-nbest --n=n --acoustic-scale=1.0 ark:<ark> ark:- | nbest-to-linear` for every entry of the table, as a list of
    dict(words, ali, graph, acoustic) in key order (<key>-1, <key>-2, ...)."""
    return [p for (_, start, finals, arcs) in read_compact_lattice_table(Path(ark).read_bytes()) for p in nbest(start, finals, arcs, n)]


def nbest_text(table: bytes, n: int) -> bytes:
    """The bytes `lattice-to-nbest --n=n --acoustic-scale=1.0 ark:- ark:- | nbest-to-linear ark:- ark:/dev/null ark,t:-` prints."""
    lines = []
    for key, start, finals, arcs in read_compact_lattice_table(table):
        for k, p in enumerate(nbest(start, finals, arcs, n), 1):
            lines.append(f"{key}-{k} " + "".join(f"{w} " for w in p["words"]) + "\n")
    return "".join(lines).encode()
