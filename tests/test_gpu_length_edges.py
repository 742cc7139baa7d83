"""GPU tests at the utterance-length edges (tests/length_cases.py): every variant at every length -- one frame up, the streaming
chunk and tick edges, clips without a frame, the online CMVN's edges -- against what the reference's binaries gave
(tests/golden/lengths/<variant>.npz, oracle/gen_length_golden.py; the CPU oracle is pinned to the same files by
tests/test_length_edges_cpu.py).  Offline one utterance per call, streams in three deliveries, one ragged batch per variant, many
runs of one to three frames under the zamia-size model's wide GEMM tiles, partial results of short streams.

A variant's test checks all of its lengths and reports every failing one; every message names the variant and n."""
import numpy as np
import pytest

from tests import length_cases as lc
from tests.test_gpu_parity import FEAT_TOL, FEAT_TOL_P99, IVEC_TOL, LOGLIKE_TOL, parse_nbest

pytestmark = pytest.mark.gpu

NBEST = 5
COST_RTOL, COST_ATOL = 2e-4, 2e-3


class Variant:
    """Files, golden, models (by options) and the one-utterance-per-call decodes of a variant, made once per module."""

    def __init__(self, name, root):
        self.name = name
        self.model_dir, self.graph_dir, self.pcm = lc.build_variant_files(name, root)
        self.g = lc.load_golden(name)
        self.ns = list(lc.lengths(name))
        assert [int(x) for x in self.g["lengths"]] == self.ns
        self.opts = dict(lc.VARIANTS[name].get("opts", {}))
        self.has_iv = lc.VARIANTS[name]["spec"].get("ivector_dim", 1) != 0
        self._models, self._single, self._stream = {}, {}, {}
        self.maxima = dict(features=0.0, ivector=0.0, loglikes=0.0)

    def model(self, **extra):
        from rhasspy_speech_amd import _lib
        k = tuple(sorted(extra.items()))
        if k not in self._models:
            o = dict(keep_intermediates=1)
            o.update(self.opts)
            o.update(extra)
            self._models[k] = _lib.Model(self.model_dir, self.graph_dir, _lib.default_opts(**o))
        return self._models[k]

    def clip(self, n):
        return self.pcm[:n]

    def has_frames(self, n, mode="offline"):
        return int(self.g[f"{lc.key(n)}_{mode}_status"]) == 0

    def single(self, n):
        """The clip decoded alone (5-best)."""
        if n not in self._single:
            self._single[n] = self.model().decode_batch([self.clip(n)], nbest=NBEST)
        return self._single[n]

    def single_stream(self, n):
        """The clip as a stream alone: one accept of everything, then finish (5-best)."""
        from rhasspy_speech_amd import _lib
        if n not in self._stream:
            st = _lib.Stream(self.model())
            st.accept(self.clip(n))
            self._stream[n] = st.finish(nbest=NBEST)
            st.close()
        return self._stream[n]

    def note(self, what, d):
        self.maxima[what] = max(self.maxima[what], float(d))


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Variant(name, tmp_path_factory.mktemp(name))
        return built[name]

    yield get
    for name, v in built.items():      # the largest differences from the reference seen in this run
        print(f"\nlength edges {name}: " + " ".join(f"max|d {k}|={d:.2e}" for k, d in v.maxima.items()))


class Failures:
    """Runs a check per length and keeps every failure."""

    def __init__(self, V):
        self.V, self.bad, self.ran = V, [], 0

    def run(self, n, what, fn):
        self.ran += 1
        try:
            fn()
        except Exception as e:      # noqa: BLE001 (an RsError at an edge is a finding like a wrong number)
            self.bad.append(f"{self.V.name} n={n} ({lc.num_frames(self.V.name, n)} frames) {what}: {type(e).__name__}: {str(e).strip()[:400]}")

    def done(self):
        assert not self.bad, "\n".join([f"{len(self.bad)} of {self.ran} checks failed"] + self.bad)


def _raises_no_frames(V, n, mode, res, u):
    """Class D: the reference's status is not 0 and the library's message is the reference's."""
    from rhasspy_speech_amd import _lib
    tag = f"{V.name} n={n} {mode}"
    assert res.num_frames(u) == 0, tag
    with pytest.raises(_lib.RsError) as ei:
        res.words(u)
    msg, ref = str(ei.value).strip(), lc.reference_error(V.g, n, mode)
    assert msg == ref, f"{tag}: library says {msg!r}, the reference {ref!r}"


def _check_nbest(V, n, mode, res, u):
    tag, k = f"{V.name} n={n} {mode}", f"{lc.key(n)}_{mode}"
    text = bytes(V.g[f"{k}_nbest_text"])
    ref = parse_nbest(text)
    assert res.num_hyps(u) == len(ref), f"{tag}: {res.num_hyps(u)} hypotheses, the reference has {len(ref)}"
    got = [res.words(u, j) for j in range(len(ref))]
    assert got == ref, f"{tag}: words {got} != {ref}"
    gc = np.array([res.costs(u, j)[0] for j in range(len(ref))])
    ac = np.array([res.costs(u, j)[1] for j in range(len(ref))])
    np.testing.assert_allclose(gc, V.g[f"{k}_graph_cost"], rtol=COST_RTOL, atol=COST_ATOL, err_msg=f"{tag}: graph costs")
    np.testing.assert_allclose(ac, V.g[f"{k}_acoustic_cost"], rtol=COST_RTOL, atol=COST_ATOL, err_msg=f"{tag}: acoustic costs")
    assert res.text(u).split() == text.split(), f"{tag}: text {res.text(u)!r} != {text!r}"


def check_golden(V, n, mode, res, u=0, nbest=True, features=True):
    """Utterance u of `res` (the clip of n samples, decoded offline or as a stream) against the reference."""
    tag, k, g = f"{V.name} n={n} {mode}", f"{lc.key(n)}_{mode}", V.g
    if not V.has_frames(n, mode):
        return _raises_no_frames(V, n, mode, res, u)
    assert res.num_frames(u) == int(g[f"{k}_num_frames"]), f"{tag}: {res.num_frames(u)} frames, the reference has {int(g[f'{k}_num_frames'])}"
    if features:
        want = g[f"{lc.key(n)}_input"]           # (the network's input: the same frames offline and streamed)
        feats = res.matrix(u, 0)
        assert feats.shape == want.shape, f"{tag}: features {feats.shape} != {want.shape}"
        fd = np.abs(feats - want)
        V.note("features", fd.max())
        assert fd.max() < FEAT_TOL and np.quantile(fd, 0.99) < FEAT_TOL_P99, f"{tag}: features off by {fd.max()} (p99 {np.quantile(fd, 0.99)})"
    if V.has_iv:
        want = g[f"{k}_ivector"]                 # offline (1, D); a stream: one row per chunk
        iv = res.matrix(u, 1)
        assert iv.shape == want.shape, f"{tag}: iVectors {iv.shape} != {want.shape}"
        d = np.abs(iv - want).max()
        V.note("ivector", d)
        assert d < IVEC_TOL, f"{tag}: iVector off by {d}"
    rows = lc.stored_rows(g, n, mode, res.num_frames(u))
    ll = res.matrix(u, 2)
    assert ll.shape[0] == res.num_frames(u) and ll[rows].shape == g[f"{k}_loglikes"].shape, f"{tag}: log-likelihoods {ll.shape}"
    d = np.abs(ll[rows] - g[f"{k}_loglikes"]).max()
    V.note("loglikes", d)
    assert d < LOGLIKE_TOL, f"{tag}: log-likelihoods off by {d}"
    if nbest:
        _check_nbest(V, n, mode, res, u)


def same_bits(V, n, what, a, ua, b, ub, kinds=(0, 1, 2)):
    """Two results of the same clip: equal bit for bit."""
    tag = f"{V.name} n={n} {what}"
    assert a.num_frames(ua) == b.num_frames(ub), tag
    if a.num_frames(ua) == 0:
        return
    for kind in kinds:
        if kind == 1 and not V.has_iv:
            continue
        x, y = a.matrix(ua, kind), b.matrix(ub, kind)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{tag}: matrix {kind} differs"
    assert a.num_hyps(ua) == b.num_hyps(ub), tag
    for j in range(a.num_hyps(ua)):
        assert a.words(ua, j) == b.words(ub, j), f"{tag}: words of hypothesis {j}"
        assert a.costs(ua, j) == b.costs(ub, j), f"{tag}: costs of hypothesis {j}: {a.costs(ua, j)} != {b.costs(ub, j)}"
    assert a.text(ua) == b.text(ub), tag


ALL = list(lc.VARIANTS)


# ------------------------------------------------------------------------------------------------ offline, one utterance per call
@pytest.mark.parametrize("variant", ALL)
def test_offline_one_utterance_per_call(variants, variant):
    V = variants(variant)
    f = Failures(V)

    def one(n):
        res = V.single(n)
        check_golden(V, n, "offline", res)
        if V.has_frames(n):
            best = V.model().decode_batch([V.clip(n)], nbest=1)       # the device traceback
            assert best.num_hyps(0) == 1 and best.words(0) == res.words(0, 0), f"{V.name} n={n}: traceback {best.words(0)} != first hypothesis {res.words(0, 0)}"
    for n in V.ns:
        f.run(n, "offline", lambda: one(n))
    f.done()


# ------------------------------------------------------------------------------------------------ streams, three deliveries
def _deliver(V, n, how):
    from rhasspy_speech_amd import _lib
    clip = V.clip(n)
    if how == "whole":
        return V.single_stream(n)
    st = _lib.Stream(V.model(stream_min_ticks=1) if how == "ticks" else V.model())
    step = lc.TICK if how == "ticks" else 777
    for i, pos in enumerate(range(0, n, step)):
        st.accept(clip[pos:pos + step])
        if how == "ticks" or i % 3 == 2:
            st.advance()
    res = st.finish(nbest=NBEST)
    st.close()
    return res


@pytest.mark.parametrize("variant", ALL)
def test_streams_in_three_deliveries(variants, variant):
    """One accept of everything; 1024-sample accepts with an advance after each (stream_min_ticks = 1: every tick is worked on as it
    arrives); 777-sample accepts with an advance after every third.  Each held to the reference's streaming golden, and the three
    equal bit for bit."""
    V = variants(variant)
    f = Failures(V)

    def one(n):
        got = {how: _deliver(V, n, how) for how in ("whole", "ticks", "777")}
        for how, res in got.items():
            check_golden(V, n, "stream", res)
        for how in ("ticks", "777"):
            same_bits(V, n, f"stream delivered as {how} vs whole", got[how], 0, got["whole"], 0)
    for n in V.ns:
        f.run(n, "stream", lambda: one(n))
    f.done()


# ------------------------------------------------------------------------------------------------ one ragged batch per variant
@pytest.mark.parametrize("variant", ALL)
def test_ragged_batch_of_every_length(variants, variant):
    """Every length of the variant, the clips without a frame included, in one decode_batch in a shuffled order: each utterance
    held to its golden, log-likelihoods and costs bit for bit those of the clip decoded alone; the same set as streams through one
    finish_streams."""
    from rhasspy_speech_amd import _lib
    V = variants(variant)
    order = [V.ns[i] for i in np.random.default_rng(20 + ALL.index(variant)).permutation(len(V.ns))]
    f = Failures(V)
    batch = V.model().decode_batch([V.clip(n) for n in order], nbest=NBEST)
    for u, n in enumerate(order):
        f.run(n, "in the ragged batch", lambda: check_golden(V, n, "offline", batch, u))
        f.run(n, "ragged batch vs alone", lambda: same_bits(V, n, "batch vs alone", batch, u, V.single(n), 0))
    streams = [_lib.Stream(V.model()) for _ in order]
    for st, n in zip(streams, order):
        st.accept(V.clip(n))
    sbatch = _lib.finish_streams(streams, nbest=NBEST)
    for st in streams:
        st.close()
    for u, n in enumerate(order):
        f.run(n, "in finish_streams", lambda: check_golden(V, n, "stream", sbatch, u))
        f.run(n, "finish_streams vs alone", lambda: same_bits(V, n, "streams vs alone", sbatch, u, V.single_stream(n), 0))
    f.done()


# ------------------------------------------------------------------------------------------------ many short runs under wide tiles
def _short_run_batch(V):
    """320 clips of the zamia-size variant: at least 200 of one to three frames, a few of 29, runs of up to three clips without a
    frame in between.  Returns the sample counts."""
    rng = np.random.default_rng(8)
    short = [lc.samples(V.name, T) for T in (1, 2, 3)]
    longer = [lc.samples(V.name, T) for T in (5, 8, 12, 24, 25)]
    ns = []
    while len(ns) < 320:
        r = rng.random()
        if r < 0.72:
            ns.append(short[int(rng.integers(0, 3))])
        elif r < 0.80:
            ns.extend([399] * int(rng.integers(1, 4)))
        elif r < 0.96:
            ns.append(longer[int(rng.integers(0, len(longer)))])
        else:
            ns.append(lc.samples(V.name, 29))
    ns = ns[:320]
    T = np.array([lc.num_frames(V.name, n) for n in ns])
    assert (np.logical_and(T >= 1, T <= 3)).sum() >= 200 and (T == 29).sum() >= 3 and (T == 0).sum() >= 20
    assert any(ns[i:i + 3] == [399] * 3 for i in range(len(ns)))
    return ns


def test_many_short_runs_under_wide_tiles(variants, monkeypatch):
    """Row lists whose runs hold one to three entries on the model with 128/160-row GEMM tiles: a tile of 128 list entries then
    crosses a hundred utterance boundaries (SpanOfRuns, call_plan.cc).  Every utterance with frames is held to its golden -- in the
    kernels such a call takes by itself and with the wide tiles forced on every launch (RS_GEMM_B3J=2, both tile heights), which a
    batch a few times larger takes by itself -- and the forced runs equal the first bit for bit.  512 copies of the one-frame clip."""
    V = variants("V8")
    ns = _short_run_batch(V)
    f = Failures(V)
    pcms = [V.clip(n) for n in ns]
    res = V.model().decode_batch(pcms, nbest=NBEST)
    assert res.num_utts == len(ns)
    for u, n in enumerate(ns):
        f.run(n, f"utterance {u} of 320", lambda: check_golden(V, n, "offline", res, u))
    for mr in ("4", "5"):
        monkeypatch.setenv("RS_GEMM_B3J", "2")
        monkeypatch.setenv("RS_GEMM_B3J_MR", mr)
        wide = V.model().decode_batch(pcms, nbest=NBEST)
        monkeypatch.delenv("RS_GEMM_B3J")
        monkeypatch.delenv("RS_GEMM_B3J_MR")
        for u, n in enumerate(ns):
            f.run(n, f"utterance {u} of 320, {32 * int(mr)}-row tiles", lambda: check_golden(V, n, "offline", wide, u))
            f.run(n, f"utterance {u} of 320, {32 * int(mr)}-row tiles vs default", lambda: same_bits(V, n, "wide tiles vs default", wide, u, res, u, kinds=(2,)))
    n1 = lc.samples(V.name, 1)
    copies = V.model().decode_batch([V.clip(n1)] * 512, nbest=NBEST)
    for u in range(512):
        f.run(n1, f"copy {u} of 512", lambda: check_golden(V, n1, "offline", copies, u))
    assert "range_retries=0 precision_retries=0" in V.model().describe(), V.model().describe()
    f.done()


def test_many_short_runs_subsampled_are_every_third_row(variants, tmp_path):
    """The same 320 clips with frame_subsampling_factor = 3 (T = 1, 2, 3, 4 give 1, 1, 1, 2 decoder frames; the upper layers run
    through strided row lists of one or two entries per utterance): bit for bit rows [::3] of the dense run, on the zamia-size model
    without dither (whose noise would follow the factor through the reference's rand() count)."""
    from rhasspy_speech_amd import _lib, synth
    from tests import cases
    V = variants("V8")
    ns = _short_run_batch(V)
    case = dict(lc.case("V8"), spec=dict(dither=0.0))
    spec = cases.case_spec(case)
    synth.write_model_dir(tmp_path / "model", spec)
    pcms = [V.clip(n) for n in ns]
    out = {}
    for fsf in (1, 3):
        model = _lib.Model(tmp_path / "model", V.graph_dir, _lib.default_opts(keep_intermediates=1, frame_subsampling_factor=fsf))
        out[fsf] = model.decode_batch(pcms)
    f = Failures(V)

    def one(u, n):
        T = lc.num_frames(V.name, n)
        assert out[1].num_frames(u) == T and out[3].num_frames(u) == (T + 2) // 3, f"V8 n={n}: frames {out[1].num_frames(u)}, {out[3].num_frames(u)}"
        if T == 0:
            return
        for kind in (0, 1):
            assert np.array_equal(out[3].matrix(u, kind), out[1].matrix(u, kind)), f"V8 n={n}: matrix {kind}"
        assert np.array_equal(out[3].matrix(u, 2), out[1].matrix(u, 2)[::3]), f"V8 n={n}: subsampled log-likelihoods are not rows [::3] of the dense ones"
    for u, n in enumerate(ns):
        f.run(n, f"utterance {u} of 320", lambda: one(u, n))
    f.done()


# ------------------------------------------------------------------------------------------------ partials on short streams
@pytest.mark.parametrize("variant", ["V1", "V4", "V6"])
def test_partials_on_short_streams(variants, variant):
    """partial() after every 1024-sample accept of the class A and B clips: the best path over the frames searched so far against
    the sequential oracle on the library's own log-likelihoods (tests/test_gpu_stream_partial.py); a stream with no decoded frame
    yet gives no words, no frames and zero cost; the finish after the partials still equals the golden."""
    from oracle import pipeline
    from rhasspy_speech_amd import _lib
    from tests.test_gpu_stream_partial import COST_ATOL as P_ATOL, COST_RTOL as P_RTOL, _oracle_best
    V = variants(variant)
    orc = pipeline.Oracle(V.model_dir, V.graph_dir, **V.opts)
    f = Failures(V)

    def one(n):
        tag = f"{V.name} n={n}"
        st = _lib.Stream(V.model(stream_min_ticks=1))
        parts = []
        for pos in range(0, n, lc.TICK):
            st.accept(V.clip(n)[pos:pos + lc.TICK])
            r = st.partial()
            assert r.num_utts == 1 and r.num_hyps(0) == 1, tag
            parts.append((r.num_frames(0), r.words(0), r.costs(0)))
            r.close()
        res = st.finish(nbest=NBEST)
        st.close()
        check_golden(V, n, "stream", res)
        ll = res.matrix(0, 2)
        last = 0
        for frames, words, costs in parts:
            assert last <= frames <= ll.shape[0], f"{tag}: partial over {frames} frames after one over {last}"
            last = frames
            if frames == 0:
                assert words == [] and costs == (0.0, 0.0), f"{tag}: partial before any frame: {words} {costs}"
                continue
            best = _oracle_best(orc, ll, frames)
            assert words == best.words, f"{tag}: partial over {frames} frames: {words} != {best.words}"
            np.testing.assert_allclose(costs, (best.graph_cost, best.acoustic_cost), rtol=P_RTOL, atol=P_ATOL, err_msg=f"{tag}: partial over {frames} frames")
    for n, cls in lc.lengths(variant).items():
        if "A" in cls or "B" in cls:
            f.run(n, "partials", lambda: one(n))
    f.done()
