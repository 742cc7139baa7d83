"""tests/gemm_shape_cases.py without a GPU.

  1. The real planner gives every case the launches the table claims: tests/host/gemm_launch_check.cc, built with the host compiler
     under the address and undefined-behaviour sanitizers and run as a child, is handed one descriptor per (case, op) -- written
     from the case module's restatement of the net, the row lists and the operand images -- prints the `gemm_launch:` line
     DescribeGemmLaunchLine makes for it and asserts that the planned grid covers every (row, column tile) once.
  2. Every `case` label of the four dispatch switches is claimed by a row of the table or listed as unreachable, and nothing is both:
     a newly added instantiation fails here until it has a row.
  3. The restated op list is the one the library compiles the net to (the `op:` and `halo:` lines of a model loaded on the CPU).
  4. The oracle the GPU tests lean on does not rest on itself: oracle.pipeline.Nnet3.forward with float64 products against a plain
     float64 evaluation of each net written here from the spec (explicit time indices, no descriptor evaluator), two random inputs.
     Bound 1e-5 absolute: the oracle stores every layer's output as float32 (2^-24 relative, activations of a few units, at most ten
     layers, BatchNorm gains up to 3.2) -- about 1e-6 -- and 1e-5 is a tenth of the 1e-4 the GPU log-likelihoods are held to."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from . import gemm_shape_cases as gsc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """{case: the lines the real planner prints for the case's descriptors}"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("gemm_shapes")
    exe = tmp / "gemm_launch_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "tests" / "host" / "gemm_launch_check.cc"), str(CSRC / "gemm_launch.cc"), "-o", str(exe)], check=True)
    owners, text = [], []
    for name, case in gsc.CASES.items():
        for d in gsc.descriptors(case).values():
            owners.append(name)
            text.append(d)
    (tmp / "descriptors.txt").write_text("\n".join(text) + "\n")
    p = subprocess.run([str(exe), str(tmp / "descriptors.txt")], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(owners)
    out = {name: [] for name in gsc.CASES}
    for name, line in zip(owners, lines):
        out[name].append(line)
    return out


@pytest.mark.parametrize("name", list(gsc.CASES))
def test_the_planner_gives_the_case_its_launches(planned, name):
    assert planned[name] == gsc.expected_lines(gsc.CASES[name])


def _claimed():
    return {gsc.label_of(" " + v) for c in gsc.CASES.values() for v in c["expect"].values()}


def test_every_dispatch_label_has_a_case_or_a_reason():
    labels = gsc.dispatch_labels()
    assert len(labels) == 15 + 6 + 6 + 11
    claimed = _claimed()
    assert not claimed & set(gsc.UNREACHABLE), claimed & set(gsc.UNREACHABLE)
    assert set(gsc.UNREACHABLE) <= set(labels) and claimed <= set(labels)
    missing = [l for l in labels if l not in claimed and l not in gsc.UNREACHABLE]
    assert not missing, missing
    assert all(len(reason) > 40 for reason in gsc.UNREACHABLE.values())


def test_a_deleted_row_is_noticed(monkeypatch):
    """The coverage test bites: without the one row that launches GemmKernelB3<3, false, 2> the label is reported."""
    rows = [n for n, c in gsc.CASES.items() if any(" B3<3,0,2> " in " " + v for v in c["expect"].values())]
    assert len(rows) == 1
    monkeypatch.delitem(gsc.CASES, rows[0])
    with pytest.raises(AssertionError, match="B3<3,0,2>"):
        test_every_dispatch_label_has_a_case_or_a_reason()


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    from rhasspy_speech_amd import synth
    root = tmp_path_factory.mktemp("gemm_shape_nets")
    built = {}

    def get(net):
        if net not in built:
            spec = gsc.spec_of(net)
            synth.write_model_dir(root / net / "model", spec)
            synth.make_grammar_graph(root / net / "graph", spec)
            built[net] = (root / net / "model", root / net / "graph")
        return built[net]

    return get


@pytest.mark.parametrize("net", list(gsc.NETS))
def test_the_restated_ops_are_the_librarys(model_dirs, net):
    from rhasspy_speech_amd import _lib
    spec = gsc.spec_of(net)
    ops = gsc.net_ops(spec)
    text = _lib.Model(*model_dirs(net), _lib.default_opts(keep_intermediates=1)).describe().splitlines()
    got = [l for l in text if l.startswith("op: ")]
    assert len(got) == len(ops)
    buf = {"input": 0, "ivector": -1}          # source -> buffer number, learnt at a source's first reader: one number each
    for line, o in zip(got, ops):
        m = re.fullmatch(r"op: gemm (\S+) out_dim=(\d+) k=(\d+) segs=((?:\[-?\d+:-?\d+:\d+\])+)(?: residual=0\.66\*\[(\d+)\])? stages=(\d+)", line)
        assert m, line
        assert (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(6))) == (o["name"], o["n"], sum(n for _, _, n in o["segs"]), o["stages"]), line
        segs = [tuple(int(v) for v in f.split(":")) for f in m.group(4).strip("[]").split("][")]
        sources = [(s, b) for (s, _, _), (b, _, _) in zip(o["segs"], segs)] + ([(o["res"], int(m.group(5)))] if o["res"] else [])
        assert (m.group(5) is not None) == (o["res"] is not None), line
        assert [(off, n) for _, off, n in segs] == [(off, n) for _, off, n in o["segs"]], line
        for s, b in sources:
            assert buf.setdefault(s, b) == b, (line, s, buf)
    assert len(set(buf.values())) == len(buf), buf
    _, L, R = gsc.extents(ops)
    if spec.ivector_dim:
        L, R = max(L, spec.splice_left), max(R, spec.splice_right)
    assert f"halo: L={L} R={R}" in text


# ---------------------------------------------------------------------------------------------- the oracle against plain float64
def _plain_float64(spec, comps, feats, ivector):
    """The net of synth.build_nnet(spec) on frames [0, T): every layer on the explicit time range its readers need, input frames
    clamped to the utterance, float64 throughout."""
    T = feats.shape[0]
    ops = gsc.net_ops(spec)
    _, L, R = gsc.extents(ops)
    f = lambda name, key: np.asarray(comps[name].fields[key], np.float64)
    t0 = -L                                                   # time of row 0 of `x`
    x = feats[np.clip(np.arange(-L, T + R), 0, T - 1)].astype(np.float64)

    def splice(x, t0, offs):
        lo, hi = t0 - min(offs), t0 + x.shape[0] - max(offs)          # times every offset can be read at
        return np.concatenate([x[lo + o - t0:hi + o - t0] for o in offs], axis=1), lo

    def batchnorm(name, y):
        mean, var = f(name, "<StatsMean>"), f(name, "<StatsVar>")
        eps, rms = float(comps[name].fields["<Epsilon>"]), float(comps[name].fields["<TargetRms>"])
        scale = rms / np.sqrt(var + eps)
        return (y - mean[None, :]) * scale[None, :]

    a, t0 = splice(x, t0, spec.lda_offsets)
    if spec.ivector_dim:
        a = np.concatenate([a, np.tile(ivector.astype(np.float64)[None, :], (a.shape[0], 1))], axis=1)
    x = a @ f("lda", "<LinearParams>").T + f("lda", "<BiasParams>")[None, :]
    for li, offs in enumerate(spec.layer_offsets, start=1):
        if spec.tdnnf and li > 1:
            prev, prev_t0 = x, t0
            lo_offs = [int(o) for o in comps[f"tdnnf{li}.linear"].fields["<TimeOffsets>"]]
            a, t0 = splice(x, t0, lo_offs)
            x = a @ f(f"tdnnf{li}.linear", "<LinearParams>").T
            ro_offs = [int(o) for o in comps[f"tdnnf{li}.affine"].fields["<TimeOffsets>"]]
            a, t0 = splice(x, t0, ro_offs)
            x = a @ f(f"tdnnf{li}.affine", "<LinearParams>").T + f(f"tdnnf{li}.affine", "<BiasParams>")[None, :]
            x = batchnorm(f"tdnnf{li}.batchnorm", np.maximum(x, 0.0))
            if prev.shape[1] == x.shape[1]:
                x = float(np.float32(0.66)) * prev[t0 - prev_t0:t0 - prev_t0 + x.shape[0]] + x
            continue
        a, t0 = splice(x, t0, offs)
        x = a @ f(f"tdnn{li}.affine", "<LinearParams>").T + f(f"tdnn{li}.affine", "<BiasParams>")[None, :]
        x = batchnorm(f"tdnn{li}.batchnorm", np.maximum(x, 0.0))
    x = x @ f("prefinal-chain.affine", "<LinearParams>").T + f("prefinal-chain.affine", "<BiasParams>")[None, :]
    x = batchnorm("prefinal-chain.batchnorm", np.maximum(x, 0.0))
    x = x @ f("output.affine", "<LinearParams>").T + f("output.affine", "<BiasParams>")[None, :]
    assert t0 == 0 and x.shape[0] == T
    return x


@pytest.mark.parametrize("net", list(gsc.NETS))
def test_the_float64_oracle_is_a_plain_float64_evaluation(model_dirs, net, monkeypatch):
    from oracle import pipeline
    spec = gsc.spec_of(net)
    orc = pipeline.Oracle(*model_dirs(net))
    monkeypatch.setattr(pipeline.Nnet3, "matmul", staticmethod(lambda x, wt: (x.astype(np.float64) @ wt.astype(np.float64)).astype(np.float32)))
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        T = 57
        feats = (rng.standard_normal((T, spec.num_ceps)) * 12.0).astype(np.float32)
        iv = rng.standard_normal(spec.ivector_dim).astype(np.float32) if spec.ivector_dim else None
        rows = None if iv is None else np.tile(iv[None, :], (T + 2 * orc.nnet.halo, 1))
        got = orc.nnet.forward(feats, rows)
        want = _plain_float64(spec, orc.nnet.nf.components, feats, iv)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{net} seed {seed}: max|oracle - float64| = {err:.3g}, max|loglike| = {np.abs(want).max():.3g}")
        assert err <= 1e-5, (net, seed, err)
