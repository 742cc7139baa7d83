#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- golden vectors for the n-best lister of tests/lattice_io.py (build container only).

Raw lattices drawn from fixed seeds (tests/lattice_io.random_raw_lattice) are determinised and written as CompactLattice
table entries by rs_lattice_entry_from_raw (host code, no GPU); the REFERENCE's `lattice-to-nbest | nbest-to-linear`
(oracle/_ref, built by oracle/build_ref.sh) lists their paths.  The lists, and the text one table of several entries gives,
are committed as tests/golden/lattice_tools.json; tests/test_lattice_cpu.py holds the Python lister to them, so the tests
that read the library's lattices need none of the reference's tools.
"""
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle.gen_golden import BIN  # noqa: E402
from oracle.gen_lattice_golden import paths_of_lattice  # noqa: E402
from tests.lattice_io import random_raw_lattice  # noqa: E402

OUT = REPO / "tests" / "golden" / "lattice_tools.json"
# (seed, states, n): small lattices listed whole, larger ones cut at n paths
LISTS = [(s, None, 10000) for s in range(100, 112)] + [(s, 30 + s % 10, 50) for s in range(130, 134)]
TABLE_SEEDS, TABLE_N = (120, 121, 122), 3


def lattice(seed, n_states):
    from rhasspy_speech_amd import _lib
    rng = np.random.default_rng(seed)
    n_states = n_states or int(rng.integers(5, 10))
    arcs, final = random_raw_lattice(rng, n_states, fan=3, n_words=4)
    return n_states, arcs, final, _lib


def main():
    env = dict(os.environ, PATH=f"{BIN}:{os.environ['PATH']}")
    out = {"lists": [], "table": {}}
    with tempfile.TemporaryDirectory() as td:
        ark = Path(td) / "lat.ark"
        for seed, n_states, n in LISTS:
            k, arcs, final, _lib = lattice(seed, n_states)
            ark.write_bytes(_lib.lattice_entry_from_raw(k, 0, final, arcs, 1e9, key="utt"))
            out["lists"].append(dict(seed=seed, n_states=k, n=n, paths=paths_of_lattice(ark, env, n)))
        entries = []
        for i, seed in enumerate(TABLE_SEEDS):
            k, arcs, final, _lib = lattice(seed, None)
            entries.append(_lib.lattice_entry_from_raw(k, 0, final, arcs, 1e9, key=f"utt{i}"))
        entries.append(_lib.lattice_entry_from_raw(1, 0, [0.75], [], 10.0, key="empty"))      # one path, no words
        sh = f"lattice-to-nbest --n={TABLE_N} --acoustic-scale=1.0 ark:- ark:- | nbest-to-linear ark:- ark:/dev/null ark,t:-"
        text = subprocess.run(["bash", "-c", sh], input=b"".join(entries), env=env, check=True, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE).stdout
        out["table"] = dict(seeds=list(TABLE_SEEDS), n=TABLE_N, text=text.decode())
    OUT.write_text(json.dumps(out, indent=0) + "\n")
    print(f"wrote {OUT}: {len(out['lists'])} lists, table of {len(entries)} entries")


if __name__ == "__main__":
    main()
