"""Feed-forward nnet3 graph forms without a device: how Nnet::Compile lowers the networks of tests/ff_cases.py (the `op:` lines of
the model's description against ff_cases.net_ops), the refusals at load, the CPU oracle's scale / offset components pinned to the
reference's goldens (tests/golden/ff/, written by tests/gen_ff_golden.py), the float64 restatement against the same goldens, and
what each case tells apart: the restatement with the case's feature broken moves some log-likelihood by 1e-2 at least, a hundred times
the GPU tests' tolerance.

On the commit before, the row-wise cases (ff_cases.ROWWISE) loaded as `eltwise tdnn1.renorm+tdnn1.relu ... stages=2`, `eltwise
tdnn1.renorm ... terms=2 stages=1` and the like, and every decode call on them ended in RunNnet's "row-wise component in a fused
position is not supported"; the oracle met the scale / offset components of ff_so and the chains with "oracle: unsupported component".

ff_ifdef, IfDefined(Offset(x, -2)) outside a cycle: the reference decodes it with zeros for the rows it cannot compute (see
ff_cases._net_ifdef); a plain Offset() reading is wrong on the first two frames, so the library refuses the descriptor at load.  On the
commit before it loaded and decoded those two frames wrongly (0.29 in the log-likelihoods)."""
import numpy as np
import pytest

from tests import ff_cases as ff

DECODED = [n for n in ff.CASES if n not in ff.NO_FRAME + ff.NO_LOAD]
MODELS = list({ff.model_key(n): n for n in ff.CASES if n not in ff.NO_LOAD}.values())      # one case per distinct model


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), the files written once per case."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = ff.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


# ------------------------------------------------------------------------------------------ the lowering

@pytest.mark.parametrize("name", MODELS)
def test_the_restated_ops_are_the_librarys(built, name):
    from rhasspy_speech_amd import _lib
    md, gd = built(name)[:2]
    got = ff.described_ops(_lib.Model(md, gd, _lib.default_opts(keep_intermediates=1)).describe())
    want = [ff.op_line(o) for o in ff.net_ops(ff.build_net(name), ff.fsf_of(name))]
    assert got == want, "\n" + "\n".join(f"{'  ' if a == b else '!='} {a}  |  {b}" for a, b in zip(got + [""] * len(want), want + [""] * len(got)) if a or b)


def _ops(name, **kw):
    return [ff.op_line(o) for o in ff.net_ops(ff.build_net(name), ff.fsf_of(name), **kw)]


def test_the_lowering_of_the_named_forms():
    """What the cases are there for, spelled out: the restatement itself is held to these lines."""
    o = _ops("ff_renorm128")
    assert o[:2] == ["op: gemm tdnn1.affine+tdnn1.relu out_dim=128 segs=[-1:40][0:40][1:40][0:10] stages=1",
                     "op: eltwise tdnn1.renorm out_dim=128 terms=1 stages=1"]
    assert "op: eltwise mid.renorm out_dim=48 terms=1 stages=1" in _ops("ff_range130")
    o = _ops("ff_chains128_r0")
    assert o[0].startswith("op: gemm tdnn1.affine+tdnn1.batchnorm+tdnn1.relu ") and o[0].endswith(" stages=2")
    assert o[1].startswith("op: gemm tdnn2.affine+tdnn2.relu+tdnn2.scale+tdnn2.bias+tdnn2.batchnorm ") and o[1].endswith(" stages=4")
    assert o[2].endswith(" stages=2") and o[3].endswith(" stages=6")
    assert o[4] == "op: eltwise six.relu+six.scale+six.bias+six.batchnorm+six.trunc+six.so out_dim=128 terms=1 stages=6"
    o = _ops("ff_so")
    for kind in ff._SO_KINDS:
        assert f"op: eltwise {kind}.unfused out_dim=40 terms=1 stages=1" in o
        assert f"op: gemm {kind}.b+{kind}.b_relu+{kind}.fused out_dim=40 segs=[0:40][0:40] stages=2" in o
    o = _ops("ff_sums")
    assert "op: eltwise sum3.noop out_dim=48 terms=3 stages=0" in o and "op: eltwise sum3.relu out_dim=48 terms=3 stages=1" in o
    assert "op: eltwise sum2.noop out_dim=48 terms=2 stages=0" in o and "op: eltwise sum8.relu out_dim=48 terms=8 stages=1" in o
    assert o.count("op: eltwise d.affine.sum out_dim=48 terms=3 stages=0") == 1 and "op: eltwise d.affine.sum out_dim=48 terms=1 stages=0" in o
    assert "op: gemm d.affine+d.relu out_dim=48 segs=[0:48][0:48][0:48][0:48][0:48] stages=1" in o
    assert "op: gemm d2.affine+d2.relu+res.noop out_dim=48 segs=[0:48] residual=0.66 stages=1" in o
    assert o.count("op: eltwise e.tdnn.sum out_dim=48 terms=2 stages=0") == 1      # (made once, read at the three time offsets)
    assert "op: gemm e.tdnn+e.relu out_dim=48 segs=[-1:48][-1:48][0:48][0:48][1:48][1:48] stages=1" in o
    assert o[-1] == "op: eltwise output out_dim=48 terms=2 stages=0"
    assert "op: eltwise res.noop out_dim=48 terms=2 stages=0" in _ops("ff_sums", fuse_residual=False)
    o = _ops("ff_segs16")
    assert o[1].count("[") == 16 and o[-1].startswith("op: gemm output.affine ")      # (the output-node is an alias: no op, no +output)
    o = _ops("ff_renorm128_fsf3")
    # (the third layer reads the second at -3, 0, 3: residue 0 only; the second reads the first at -1, 0, 1)
    assert [l.endswith(" rows=every-3") for l in o] == [False, False, True, True, True, True, True]


def test_a_row_wise_component_stands_alone():
    """The forms that used to load into one op and then fail every decode call."""
    o = _ops("ff_rw_relu")
    assert o[:3] == ["op: gemm tdnn1.affine out_dim=64 segs=[-1:40][0:40][1:40][0:10] stages=0", "op: eltwise tdnn1.renorm out_dim=64 terms=1 stages=1",
                     "op: eltwise tdnn1.relu out_dim=64 terms=1 stages=1"]
    assert _ops("ff_rw_bn")[1:3] == ["op: eltwise tdnn1.renorm out_dim=64 terms=1 stages=1", "op: eltwise tdnn1.batchnorm out_dim=64 terms=1 stages=1"]
    # Sum(a, b) of two layer results: the sum becomes the second GEMM's residual, the row-wise op reads it
    assert _ops("ff_rw_sum")[:3] == ["op: gemm tdnn1.affine+tdnn1.relu out_dim=64 segs=[-1:40][0:40][1:40][0:10] stages=1",
                                    "op: gemm side.affine+side.relu+tdnn1.renorm.sum out_dim=64 segs=[-1:40][0:40][1:40][0:10] residual=1 stages=1",
                                    "op: eltwise tdnn1.renorm out_dim=64 terms=1 stages=1"]
    assert _ops("ff_rw_sum", fuse_residual=False)[2:4] == ["op: eltwise tdnn1.renorm.sum out_dim=64 terms=2 stages=0", "op: eltwise tdnn1.renorm out_dim=64 terms=1 stages=1"]
    assert _ops("ff_rw_sum_off")[2:4] == ["op: eltwise tdnn1.renorm.sum out_dim=64 terms=2 stages=0", "op: eltwise tdnn1.renorm out_dim=64 terms=1 stages=1"]
    assert _ops("ff_rw_lsm_scale")[-2:] == ["op: eltwise output.log-softmax.sum out_dim=48 terms=1 stages=0",
                                           "op: eltwise output.log-softmax+output out_dim=48 terms=1 stages=1"]


@pytest.mark.parametrize("what", list(ff.REFUSED))
def test_refused_at_load_with_node_and_reason(tmp_path, what):
    from rhasspy_speech_amd import _lib
    md, gd = ff.write_case_model(ff._c(("refused", dict(what=what)), "synth:0:400"), tmp_path)[:2]
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd, _lib.default_opts())
    for part in ff.REFUSED[what]:
        assert part in str(ei.value), str(ei.value)


# ------------------------------------------------------------------------------------------ the oracle and the restatement

def parse_nbest(text: bytes):
    return [[int(x) for x in ln.split()[1:]] for ln in text.decode().splitlines() if ln.split()]


@pytest.mark.parametrize("name", DECODED)
def test_oracle_matches_reference(built, name):
    """test_oracle_golden.py's tolerances."""
    from oracle import pipeline
    g = ff.load_golden(name)
    md, gd, _, pcm = built(name)
    tr = pipeline.Oracle(md, gd).transcribe(pcm, nbest=ff.NBEST)
    assert tr.num_frames == int(g["offline_num_frames"])
    fd = np.abs(tr.feats - g["input"])
    assert fd.max() < 2e-4 and np.quantile(fd, 0.99) < 1e-4
    assert np.abs(tr.ivector - g["offline_ivector"][0]).max() < 1e-4
    assert np.abs(tr.loglikes - g["offline_loglikes"]).max() < 1e-4
    got = [p.words for p in tr.nbest]
    assert got == parse_nbest(bytes(g["offline_nbest_text"]))
    np.testing.assert_allclose([p.graph_cost for p in tr.nbest], g["offline_graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose([p.acoustic_cost for p in tr.nbest], g["offline_acoustic_cost"], rtol=2e-4, atol=2e-3)


@pytest.mark.parametrize("name", ["ff_so", "ff_chains64_r0", "ff_sums", "ff_rw_sum_off_fsf3"])
def test_oracle_streaming_matches_reference(built, name):
    from oracle import pipeline
    g = ff.load_golden(name)
    md, gd, _, pcm = built(name)
    tr = pipeline.Oracle(md, gd).transcribe_stream(pcm, nbest=ff.NBEST)
    assert np.abs(tr.ivector - g["stream_ivector"]).max() < 1e-4
    assert np.abs(tr.loglikes - g["stream_loglikes"]).max() < 1e-4
    assert tr.text() == bytes(g["stream_nbest_text"])


@pytest.fixture(scope="module")
def restated():
    done = {}

    def get(name):
        if name not in done:
            done[name] = ff.restate(name)
        return done[name]
    return get


@pytest.mark.parametrize("name", DECODED)
def test_restatement_matches_reference(restated, name):
    """The float64 network on the golden's own input rows and iVector: what is left is the reference's FP32 arithmetic."""
    g = ff.load_golden(name)
    ll = restated(name)
    assert ll.shape == g["offline_loglikes"].shape
    diff = float(np.abs(ll - g["offline_loglikes"]).max())
    print(f"{name}: float64 restatement against the reference, max abs diff {diff:.3g}")
    assert diff < 1e-4, diff


def test_the_reference_zero_fills_an_optional_input_outside_a_cycle():
    """ff_ifdef's golden against the restatement that reads IfDefined(Offset(x, -2)) as a plain Offset: the reference's context is
    (1, 1), not (3, 1); frames 0 and 1 differ by far more than any tolerance, every later frame agrees.  (The library refuses the
    model: test_refused_at_load_with_node_and_reason.)"""
    g = ff.load_golden("ff_ifdef")
    assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0 and list(g["context"]) == [1, 1]
    d = np.abs(ff.restate("ff_ifdef") - g["offline_loglikes"]).max(axis=1)
    assert d[:2].min() > 0.1 and d[2:].max() < 1e-4, (d[:4], d[2:].max())


def test_a_clip_without_a_frame_fails_in_the_reference():
    g = ff.load_golden("ff_renorm128_len0")
    assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
    assert int(ff.load_golden("ff_renorm128_len1")["offline_num_frames"]) == 1


# ------------------------------------------------------------------------------------------ what each case tells apart

SENSITIVITY = [
    # stages in the relu-batchnorm order where the network has batchnorm-relu
    ("ff_chains128_r0", dict(swap=("tdnn1.batchnorm", "tdnn1.relu"))),
    ("ff_chains64_r2", dict(swap=("tdnn3.batchnorm", "tdnn3.relu"))),
    # one term's offset, one term's scale dropped
    ("ff_sums", dict(no_offset=("sum3.noop", 0))),
    ("ff_sums", dict(no_scale=("sum3.relu", 0))),
    ("ff_sums", dict(no_offset=("sum8.relu", 3))),
    ("ff_sums", dict(no_scale=("d.affine", 2))),
    ("ff_sums", dict(no_scale=("e.tdnn", 0))),
    ("ff_sums", dict(no_scale=("output", 0))),
    ("ff_sums_fsf3", dict(no_offset=("sum2.noop", 0))),
    ("ff_rw_sum_off", dict(no_offset=("tdnn1.renorm", 0))),
    ("ff_rw_sum_off", dict(no_scale=("tdnn1.renorm", 0))),
    ("ff_rw_lsm_scale", dict(no_scale=("output.log-softmax", 0))),
    ("ff_segs16", dict(no_offset=("b.affine", 10))),
    # the normalize floor
    ("ff_renorm_floor", dict(norm_floor=False)),
    # a dim-range read from column 0
    ("ff_range65", dict(col0_zero=True)),
    ("ff_range130", dict(col0_zero=True)),
    ("ff_segs16", dict(col0_zero=True)),
    # target-rms
    ("ff_renorm128", dict(use_target_rms=False)),
    ("ff_renorm33", dict(use_target_rms=False)),
    ("ff_rw_sum", dict(use_target_rms=False)),
    # EnsureNonzero
    ("ff_so", dict(apply_ensure_nonzero=False)),
    # every other case, by the feature it is there for
    ("ff_renorm100", dict(use_target_rms=False)),
    ("ff_renorm65", dict(use_target_rms=False)),
    ("ff_renorm128_fsf3", dict(use_target_rms=False)),
    ("ff_renorm128_len1", dict(use_target_rms=False)),
    ("ff_chains128_r1", dict(swap=("tdnn4.batchnorm", "tdnn4.relu"))),
    ("ff_chains128_r2", dict(swap=("tdnn3.batchnorm", "tdnn3.relu"))),
    ("ff_chains128_r3", dict(swap=("tdnn2.batchnorm", "tdnn2.relu"))),
    ("ff_chains64_r0", dict(swap=("tdnn1.batchnorm", "tdnn1.relu"))),
    ("ff_rw_relu", dict(swap=("tdnn1.renorm", "tdnn1.relu"))),
    ("ff_rw_relu_fsf3", dict(swap=("tdnn1.renorm", "tdnn1.relu"))),
    ("ff_rw_bn", dict(swap=("tdnn1.renorm", "tdnn1.batchnorm"))),
    ("ff_rw_bn_fsf3", dict(swap=("tdnn1.renorm", "tdnn1.batchnorm"))),
    ("ff_rw_sum_fsf3", dict(use_target_rms=False)),
    ("ff_rw_sum_off_fsf3", dict(no_offset=("tdnn1.renorm", 0))),
    ("ff_rw_lsm_scale_fsf3", dict(no_scale=("output.log-softmax", 0))),
    ("ff_range130_fsf3", dict(col0_zero=True)),
    ("ff_range65_fsf3", dict(col0_zero=True)),
]


def test_every_decoded_case_has_a_sensitivity_entry():
    assert {n for n, _ in SENSITIVITY} == set(DECODED)


@pytest.mark.parametrize("name,switch", SENSITIVITY, ids=[f"{n}-{next(iter(s))}-{i}" for i, (n, s) in enumerate(SENSITIVITY)])
def test_the_case_tells_its_feature(restated, name, switch):
    ll, broken = restated(name), ff.restate(name, **switch)
    moved = float(np.abs(broken - ll).max()) if np.isfinite(broken).all() else float("inf")
    print(f"{name} {switch}: max log-likelihood change {moved:.3g}")
    assert moved >= 1e-2, (name, switch, moved)


def test_the_floor_case_has_rows_of_zeros():
    """ff_renorm_floor: every row of the second layer's relu is zero, so kSquaredNormFloor alone decides tdnn2.renorm (zeros, not
    0 / 0)."""
    g = ff.load_golden("ff_renorm_floor")
    net = ff.Float64Net(ff.build_net("ff_renorm_floor"))
    net.forward(g["input"], g["offline_ivector"][0])
    assert not net.memo["tdnn2.relu"][1].any() and not net.memo["tdnn2.renorm"][1].any()


def test_existing_models_are_written_as_before():
    """synth.write_final_mdl took a parameter: the files of two specs of tests/cases.py (tiny_u0's, tinyf_u5's) hash as they did before
    it had one, and a network handed in is written like the one build_nnet makes."""
    import hashlib
    import tempfile
    from pathlib import Path
    from rhasspy_speech_amd import synth
    tinyf = dict(tdnnf=True, with_priors=True, with_log_softmax=True, layer_offsets=((0,), (-1, 0, 1), (-1, 0, 1), (-3, 0, 3)))
    want = {(): "f3cd52d4ed52dc3e12ea4f5c597431b45e95623a5878a1f3cfea2710429f9fbf",
            tuple(sorted(tinyf)): "2b1e98c8d1b3650a688a6dfeb5b69025e7d3800f955a33dfc3f35c97c37dcaaa"}
    with tempfile.TemporaryDirectory() as td:
        for kw in ({}, tinyf):
            synth.write_final_mdl(Path(td) / "a.mdl", synth.tiny_spec(**kw))
            assert hashlib.sha256((Path(td) / "a.mdl").read_bytes()).hexdigest() == want[tuple(sorted(kw))]
        spec = synth.tiny_spec()
        synth.write_final_mdl(Path(td) / "b.mdl", spec, nnet=synth.build_nnet(spec, np.random.default_rng(spec.seed)))
        assert hashlib.sha256((Path(td) / "b.mdl").read_bytes()).hexdigest() == want[()]
