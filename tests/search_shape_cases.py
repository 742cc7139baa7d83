"""A family of graphs that puts the search on every kernel shape, closure depth and limit the planner (csrc/search_plan.cc) can
choose, shared by tests/test_search_shapes_cpu.py, tests/test_gpu_search_shapes.py and oracle/gen_search_shape_golden.py.

Every graph is a prefix-tree grammar in the layout of synth.make_grammar_hclg (phone HMMs by synth._add_phone, optional silence at
every word end) over generated sentences, padded to exact counts of states, emitting arcs and epsilon arcs:
  * filler phone chains (dead ends hanging off grammar states, without output labels) where a state count is asked for -- without
    their self-loops where the graph may have fewer than 2 emitting arcs per state;
  * extra emitting arcs between existing states (a forward transition into an existing phone state, cost 4 + log 2);
  * extra epsilon arcs (cost 5) only from states without epsilon in-arcs to states without epsilon out-arcs, so each is an epsilon
    path of length 1 whatever else the graph holds.
Depth d >= 2: at every word end the last phone state `cur` reaches the next grammar state `nxt` through a chain of d epsilon arcs
of total cost log 2 and through a one-arc shortcut of cost log 2 + 1; the optional-silence state joins the chain at its second node.
The cheapest way to every `nxt` is then its longest epsilon path: a closure that stops a round early pays 1.0 per word.
All graphs are acyclic in their epsilon arcs.  walk() restates WalkSearchGraph in Python; build() asserts its targets with it."""
from __future__ import annotations

import math
from functools import lru_cache
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from rhasspy_speech_amd import synth

SPEC_KW = dict(num_phones=40, dither=0.0)
NBEST = 5
# synth_utterance(seed, samples).  On every case, option set and clip the reference's 5-best list does not hang on the order in which
# its decoder happens to create tokens (tests/test_search_shapes_cpu.py checks that with the sequential oracle decoder), so it is
# a target for the kernels, which prune with each frame's final cutoff ("order-dependent extras")
CLIPS = ((31, 24000), (32, 8000), (34, 1200))
# ... and the one combination met while choosing the clips on which it does: with max-active binding on this 6-frame clip the
# reference keeps one token above the final cutoff of its frame and lists two more hypotheses.  Pinned as what it is.
ORDER_DEPENDENT = dict(case="depth7", options="binding", clip=(33, 1200), hyps=(5, 3))
BINDING = dict(max_active=150, min_active=100, beam=10.0)      # the binding set of test_gpu_parity.VARIANT_CASES
OPTION_SETS = {"default": {}, "binding": BINDING}
VOCAB = 48
STREAM_CASES = ("e2049", "e4097", "depth3", "depth7", "out32")
CROWDED_CASES = ("e2048_x1024", "e4096_x2048")
DEPTH_CASES = ("depth2", "depth3", "depth6", "depth7", "depth9", "depth3_s2500", "depth7_s2500")

# name: targets (S exact, or S_max with the base graph built up to it; e / x exact), then where the planner must put it:
#   reg "<nt,ke,kx>" | "none", dl "<512,ka>" | "none", eps_rounds, exact_ok, route of an n-best call (dense-rows / rows-to-tokens / tokens)
CASES: Dict[str, dict] = {
    "e2048_x1024": dict(S_max=1000, e=2048, x=1024, reg="<512,4,2>", dl="<512,6>", rounds=1, exact_ok=1, route="dense-rows"),
    "e2049": dict(S_max=1000, e=2049, x=1024, reg="<512,8,4>", dl="<512,8>", rounds=1, exact_ok=1, route="dense-rows"),
    "x1025": dict(S_max=1000, e=2048, x=1025, reg="<512,8,4>", dl="<512,8>", rounds=1, exact_ok=1, route="dense-rows"),
    "e4096_x2048": dict(S_max=2048, e=4096, x=2048, reg="<512,8,4>", dl="<512,12>", rounds=1, exact_ok=0, route="dense-rows"),
    "e4097": dict(S_max=2048, e=4097, x=2048, reg="<256,32,16>", dl="<512,16>", rounds=1, exact_ok=0, route="dense-rows"),
    "a8192_s2048": dict(S=2048, e=6144, x=2048, reg="<256,32,16>", dl="<512,16>", rounds=1, exact_ok=0, route="dense-rows"),
    "s2049": dict(S=2049, e=6144, x=2048, reg="<256,32,16>", dl="none", rounds=1, exact_ok=0, route="rows-to-tokens"),
    "e8192_x4096": dict(S_max=5000, e=8192, x=4096, reg="<256,32,16>", dl="none", rounds=1, exact_ok=0, route="rows-to-tokens"),
    "s5000": dict(S=5000, e=8000, x=1700, reg="<256,32,16>", dl="none", rounds=1, exact_ok=0, route="rows-to-tokens"),
    "s5001": dict(S=5001, e=8000, x=1700, reg="none", dl="none", rounds=0, exact_ok=0, route="tokens"),
    "a1024": dict(S_max=400, e=832, x=192, reg="<512,4,2>", dl="<512,2>", rounds=1, exact_ok=1, route="dense-rows"),
    "a1025": dict(S_max=400, e=833, x=192, reg="<512,4,2>", dl="<512,4>", rounds=1, exact_ok=1, route="dense-rows"),
    "exact_s1000_e2100": dict(S=1000, e=2100, x=400, reg="<512,8,4>", dl="<512,6>", rounds=1, exact_ok=1, route="dense-rows"),
    "exact_s1001": dict(S=1001, e=2100, x=400, reg="<512,8,4>", dl="<512,6>", rounds=1, exact_ok=0, route="dense-rows"),
    "out32": dict(S_max=1000, e=1900, x=500, first_words=32, x32=True, reg="<512,4,2>", dl="<512,6>", rounds=1, exact_ok=1, route="dense-rows",
                  max_out=(32, 32)),
    "depth0": dict(S_max=400, e=900, x=0, depth=0, reg="<512,4,2>", dl="<512,2>", rounds=0, exact_ok=1, route="dense-rows"),
    "depth2": dict(seed=2, S_max=400, e=700, x=320, depth=2, reg="<512,4,2>", dl="<512,2>", rounds=2, exact_ok=0, route="dense-rows"),
    "depth3": dict(S_max=400, e=700, x=330, depth=3, reg="<512,4,2>", dl="<512,4>", rounds=3, exact_ok=0, route="dense-rows"),
    "depth6": dict(seed=7, S_max=400, e=600, x=430, depth=6, reg="<512,4,2>", dl="<512,4>", rounds=6, exact_ok=0, route="dense-rows"),
    "depth7": dict(S_max=480, first_words=8, e=600, x=430, depth=7, reg="<512,4,2>", dl="<512,4>", rounds=-1, exact_ok=0, route="dense-rows"),
    "depth9": dict(S_max=480, first_words=8, e=600, x=430, depth=9, reg="<512,4,2>", dl="<512,4>", rounds=-1, exact_ok=0, route="dense-rows"),
    "depth3_s2500": dict(S=2500, e=4000, x=1900, depth=3, reg="<512,8,4>", dl="none", rounds=3, exact_ok=0, route="rows-to-tokens"),
    "depth7_s2500": dict(S=2500, e=3600, x=2000, depth=7, reg="<512,8,4>", dl="none", rounds=-1, exact_ok=0, route="rows-to-tokens"),
}


def spec() -> synth.ModelSpec:
    return synth.tiny_spec(**SPEC_KW)


def clips() -> List[np.ndarray]:
    return [synth.synth_utterance(seed, n) for seed, n in CLIPS]


def arc_list(fst: synth.Fst) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(src, dst, emitting) per arc in the order write_const_fst stores them, which is the order the library walks."""
    src, dst, em = [], [], []
    for s, al in enumerate(fst.arcs):
        for il, ol, _, n in sorted(al, key=lambda a: (a[0], a[1], a[3])):
            src.append(s); dst.append(n); em.append(1 if il != 0 else 0)
    return np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(em, np.int64)


def walk(fst: synth.Fst) -> Tuple[int, int, int, int, int, int]:
    """(S, in_e, in_x, eps_depth, max_out_e, max_out_x) as WalkSearchGraph finds them: eps_depth is the longest path of the epsilon
    subgraph (Kahn's order), -1 if it has a cycle, and 0 beyond 5000 states, where no kernel asks."""
    S = fst.num_states
    src, dst, em = arc_list(fst)
    out_e = np.bincount(src[em == 1], minlength=S)
    out_x = np.bincount(src[em == 0], minlength=S)
    indeg = np.bincount(dst[em == 0], minlength=S)
    depth = 0
    if S <= 5000:
        succ: List[List[int]] = [[] for _ in range(S)]
        for s, d in zip(src[em == 0].tolist(), dst[em == 0].tolist()):
            succ[s].append(d)
        indeg = indeg.tolist()
        length = [0] * S
        order = [s for s in range(S) if indeg[s] == 0]
        for s in order:      # (grows while it is walked)
            for d in succ[s]:
                length[d] = max(length[d], length[s] + 1)
                indeg[d] -= 1
                if indeg[d] == 0:
                    order.append(d)
        depth = -1 if len(order) < S else max(length)
    return S, int(em.sum()), int((em == 0).sum()), depth, int(out_e.max()), int(out_x.max())


def write_arcs_file(path: Path, fst: synth.Fst, num_pdfs: int) -> None:
    """The input of `search_plan_check --graph`: "states pdfs arcs", then "src dst emitting" per arc."""
    src, dst, em = arc_list(fst)
    with open(path, "w") as f:
        f.write(f"{fst.num_states} {num_pdfs} {len(src)}\n")
        f.write("".join(f"{s} {d} {e}\n" for s, d, e in zip(src.tolist(), dst.tolist(), em.tolist())))


def _sentences(rng: np.random.Generator, vocab: List[str], n: int, first_words: int) -> List[List[str]]:
    """n sentences of 2-4 words; the first word is one of `first_words`, each next one of 6 that follow the word before it, so a
    grammar state has at most max(first_words, 6) word arcs."""
    out = []
    for i in range(n):
        w = i % first_words if i < first_words else int(rng.integers(0, first_words))
        s = [w]
        for _ in range(int(rng.integers(1, 4))):
            w = (w * 7 + 1 + int(rng.integers(0, 6))) % len(vocab)
            s.append(w)
        out.append([vocab[k] for k in s])
    return out


class _Builder:
    def __init__(self, depth: int, variant: str):
        self.spec = spec()
        self.depth, self.variant = depth, variant
        self.fst = synth.Fst()
        self.phone_of: Dict[int, int] = {}      # phone states -> phone
        self.grammar: List[int] = []            # grammar states, where word arcs leave
        self.word_end: List[int] = []           # last phone state of every word
        self.left_out: List[Tuple[int, int]] = []      # epsilon arcs (src, dst) of the full graph that this variant leaves out

    def phone(self, src: int, phone: int, olabel: int, cost: float, self_loop: bool = True) -> int:
        if self_loop:
            st = synth._add_phone(self.fst, self.spec, src, phone, olabel, cost)
        else:
            st = self.fst.add_state()
            self.fst.add_arc(src, synth.transition_ids(self.spec, phone)[1], olabel, cost + math.log(2.0), st)
        self.phone_of[st] = phone
        return st

    def join(self, cur: int, sil: Optional[int], nxt: int) -> None:
        """cur (and the optional-silence state) reach nxt: one arc each at depth 1, the chain and its shortcut from depth 2 on."""
        f, d = self.fst, self.depth
        if d <= 1:
            f.add_arc(cur, 0, 0, math.log(2.0), nxt)
            if sil is not None:
                f.add_arc(sil, 0, 0, 0.0, nxt)
            return
        nodes = [cur] + [f.add_state() for _ in range(d - 1)] + [nxt]
        for k in range(d):
            if self.variant == "broken" and k == d - 1:      # the last link: neither cur nor the silence gets through the chain
                self.left_out.append((nodes[k], nodes[k + 1]))
                continue
            f.add_arc(nodes[k], 0, 0, math.log(2.0) / d, nodes[k + 1])
        if self.variant != "no_shortcut":
            f.add_arc(cur, 0, 0, math.log(2.0) + 1.0, nxt)
        else:
            self.left_out.append((cur, nxt))
        if sil is not None:
            f.add_arc(sil, 0, 0, 0.0, nodes[1])

    def tree(self, sentences: List[List[str]], lex: synth.Lexicon) -> None:
        f, spec, d = self.fst, self.spec, self.depth
        wid = {w: i for i, w in enumerate(lex.words)}
        root = f.add_state()
        f.start = root
        if d == 0:
            g0 = root
        else:      # optional leading silence
            g0 = f.add_state()
            f.add_arc(root, 0, 0, math.log(2.0), g0)
            s_sil = self.phone(root, lex.sil_phone, 0, math.log(2.0))
            f.add_arc(s_sil, 0, 0, 0.0, g0)
        self.grammar.append(g0)
        trie = {(): g0}
        counts: Dict[tuple, int] = {}
        for s in sentences:
            ids = tuple(wid[w] for w in s)
            for k in range(len(ids) + 1):
                counts[ids[:k]] = counts.get(ids[:k], 0) + 1
        for s in sentences:
            ids = tuple(wid[w] for w in s)
            for k in range(1, len(ids) + 1):
                pre = ids[:k]
                if pre in trie:
                    continue
                cur = trie[pre[:-1]]
                cost = -math.log(counts[pre] / counts[pre[:-1]])
                for j, ph in enumerate(lex.prons[pre[-1]]):
                    cur = self.phone(cur, ph, pre[-1] if j == 0 else 0, cost if j == 0 else 0.0)
                self.word_end.append(cur)
                if d == 0:      # no epsilon arcs at all: the word's last phone state is the next grammar state
                    nxt = cur
                else:
                    nxt = f.add_state()
                    self.join(cur, self.phone(cur, lex.sil_phone, 0, math.log(2.0)), nxt)
                self.grammar.append(nxt)
                trie[pre] = nxt
        ends: Dict[tuple, int] = {}
        for s in sentences:
            ids = tuple(wid[w] for w in s)
            ends[ids] = ends.get(ids, 0) + 1
        for ids, c in ends.items():
            f.finals[trie[ids]] = float(np.float32(-math.log(c / counts[ids])))


def _tree_counts(sentences, lex, depth) -> Tuple[int, int, int]:
    """(states, emitting arcs, epsilon arcs) of the tree of `sentences`, without building it."""
    wid = {w: i for i, w in enumerate(lex.words)}
    pres = {tuple(wid[w] for w in s[:k]) for s in sentences for k in range(1, len(s) + 1)}
    n_ph = sum(len(lex.prons[p[-1]]) for p in pres)
    if depth == 0:
        return 1 + n_ph, 2 * n_ph, 0
    per_x = 2 if depth == 1 else depth + 2
    return 3 + n_ph + len(pres) * (2 + depth - 1), 2 + 2 * n_ph + 2 * len(pres), 2 + per_x * len(pres)


@lru_cache(maxsize=None)
def build(name: str, variant: str = "full") -> Tuple[synth.Fst, synth.Lexicon]:
    """The graph of case `name` and its lexicon.  variant (depth cases): "no_shortcut" leaves the shortcuts out, "broken" the
    last link of every chain; both are built from the same sentences and padding draws as the full graph."""
    c = CASES[name]
    depth = c.get("depth", 1)
    first_words = c.get("first_words", 12)
    S_goal = c.get("S", c.get("S_max"))
    rng = np.random.default_rng(1000 + c.get("seed", 0))      # (seed: chosen so that the two longer clips decode to words)
    vocab = [f"w{i:02d}" for i in range(VOCAB)]
    lex = synth.make_lexicon([vocab], spec(), rng)
    # the largest tree within nine tenths of every target (the rest is padding); counts from the full variant, so all three agree
    pool = _sentences(rng, vocab, 4000, first_words)
    n = first_words
    while n < len(pool):
        s, e, x = _tree_counts(pool[:n + 1], lex, depth)
        if s > 0.9 * S_goal or e > 0.9 * c["e"] - (c.get("S", 0) and (c["S"] - s)) or (depth > 0 and x > 0.9 * c["x"]):
            break
        n += 1
    b = _Builder(depth, variant)
    b.tree(pool[:n], lex)
    f = b.fst
    full_x = _tree_counts(pool[:n], lex, depth)[2]      # (the variants have fewer epsilon arcs: they are padded like the full graph)
    S0, e0 = f.num_states, sum(1 for al in f.arcs for a in al if a[0] != 0)
    # filler chains to an exact state count: dead ends of up to 4 phones off the grammar states, no output labels; self-loops
    # only while the emitting-arc target has room for them
    if "S" in c:
        need = c["S"] - S0
        assert 0 <= need <= c["e"] - e0, (name, S0, e0)
        loops = min(need, c["e"] - e0 - need)      # fillers that keep their self-loop
        k = 0
        while need > 0:
            cur = b.grammar[k % len(b.grammar)]
            for j in range(min(4, need)):
                cur = b.phone(cur, int(rng.integers(2, b.spec.num_phones + 1)), 0, 2.0 if j == 0 else 0.0, self_loop=loops > 0)
                loops -= 1
                need -= 1
            k += 1
    S = f.num_states
    assert S <= S_goal, (name, S)
    # (the padding below treats the arcs a variant leaves out as present, so every variant draws the same arcs)
    pairs = {(s, a[3]) for s, al in enumerate(f.arcs) for a in al} | set(b.left_out)
    tries = 0
    # extra emitting arcs: a forward transition into an existing phone state
    out_e = [sum(1 for a in al if a[0] != 0) for al in f.arcs]
    phone_states = sorted(b.phone_of)
    need = c["e"] - sum(out_e)
    assert need >= 0, (name, sum(out_e))
    cap_e = max(4, -(-3 * c["e"] // (2 * S)))      # out-degrees stay near the mean, far below the exact kernel's 32
    while need > 0:
        s, d = int(rng.integers(0, S)), phone_states[int(rng.integers(0, len(phone_states)))]
        tries += 1
        assert tries < 10_000_000, name
        if s == d or (s, d) in pairs or out_e[s] >= cap_e:
            continue
        f.add_arc(s, synth.transition_ids(b.spec, b.phone_of[d])[1], 0, 4.0 + math.log(2.0), d)
        pairs.add((s, d)); out_e[s] += 1; need -= 1
    # extra epsilon arcs: from a state without epsilon in-arcs to one without epsilon out-arcs
    has_in = [False] * S
    out_x = [0] * S
    for s, al in enumerate(f.arcs):
        for a in al:
            if a[0] == 0:
                out_x[s] += 1; has_in[a[3]] = True
    for s, d in b.left_out:
        out_x[s] += 1; has_in[d] = True
    need = c["x"] - full_x
    assert need >= 0 and (depth > 0 or c["x"] == 0), (name, full_x)
    cap_x = max(4, -(-3 * c["x"] // S))
    if c.get("x32"):      # one state with 32 epsilon out-arcs: the last phone state of the first word
        s = b.word_end[0]
        assert not has_in[s]
        while out_x[s] < 32:
            d = b.grammar[int(rng.integers(0, len(b.grammar)))]
            if d == s or (s, d) in pairs or out_x[d] > 0:
                continue
            f.add_arc(s, 0, 0, 5.0, d)
            pairs.add((s, d)); out_x[s] += 1; has_in[d] = True; need -= 1
    assert need >= 0, name
    while need > 0:
        s, d = int(rng.integers(0, S)), int(rng.integers(0, S))
        tries += 1
        assert tries < 10_000_000, name
        if s == d or (s, d) in pairs or has_in[s] or out_x[d] > 0 or out_x[s] >= cap_x:
            continue
        f.add_arc(s, 0, 0, 5.0, d)
        pairs.add((s, d)); out_x[s] += 1; has_in[d] = True; need -= 1
    if variant == "full":
        got = walk(f)
        want_depth = depth if S <= 5000 else 0
        assert got[1:4] == (c["e"], c["x"], want_depth) and (got[0] == c["S"] if "S" in c else got[0] <= c["S_max"]), (name, got)
        if "max_out" in c:
            assert got[4:] == c["max_out"], (name, got)
        if c["exact_ok"]:
            assert got[4] <= 32 and got[5] <= 32, (name, got)
    return f, lex


def search_line(name: str, crowded_at: int, dense_ok: int = 1) -> str:
    """The `search:` line of rs_model_describe for case `name` (tests/test_search_shapes_cpu.py holds it to the real planner)."""
    c = CASES[name]
    S, e, x, depth, mo_e, mo_x = walk(build(name)[0])
    return (f"search: states={S} arcs_e={e} arcs_x={x} eps_depth={depth} max_out={mo_e},{mo_x} reg={c['reg']} eps_rounds={c['rounds']} "
            f"exact_ok={c['exact_ok']} dense_ok={dense_ok} dense_lattice={c['dl']} crowded_at={crowded_at}")


def write_graph(name: str, graph_dir: Path, variant: str = "full") -> synth.Fst:
    fst, lex = build(name, variant)
    synth.write_graph_dir(graph_dir, fst, lex)
    return fst
