"""Models of sampling rates other than 16 kHz without a GPU: oracle/pipeline.py against what the reference's binaries gave for the
cases of tests/rate_cases.py (tests/golden/rates/, written by tests/gen_rate_golden.py) -- so that the GPU tests may hold the library's
streams to the oracle's -- and the host side of the feature: the table builder's padded sizes, the model's rate through the C ABI,
the stream binary's --samp-freq, the synthetic model writer.

Tolerances are tests/test_oracle_golden.py's: rows 2e-4 (99 % of them 1e-4), iVectors and log-likelihoods 1e-4, costs rtol 2e-4 +
atol 2e-3, words equal."""
import hashlib
import json

import numpy as np
import pytest

from tests import rate_cases as rc


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = rc.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


@pytest.fixture(scope="module")
def oracles(built, tmp_path_factory):
    done = {}

    def get(name):
        if name not in done:
            md, gd, _, pcm = built(name)
            done[name] = (rc.make_oracle(name, md, gd, tmp_path_factory.mktemp(name + "_oracle")), pcm)
        return done[name]
    return get


def parse_nbest(text: bytes):
    return [[int(x) for x in ln.split()[1:]] for ln in text.decode().splitlines() if ln.split()]


def test_goldens_are_there_for_every_case():
    for name, case in rc.CASES.items():
        g = rc.load_golden(name)
        assert bytes(g["case_json"]).decode() == json.dumps(case, sort_keys=True), name      # (made from this table)
        if name == rc.NO_FRAME:
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        keys = {"input", "rand_calls", "offline_loglikes"} | {f"{m}_{k}" for m in ("offline", "stream")
                                                              for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames")}
        if case["spec"].get("ivector_dim", 1) > 0:
            keys |= {"offline_ivector"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        n = int(case["audio"].split(":")[2])
        fsf = int(case.get("conf_opts", {}).get("frame-subsampling-factor", 1))
        T = rc.num_frames(name, n)
        assert g["input"].shape == (T, rc.feat_dim(name)) and T >= 1
        assert int(g["offline_num_frames"]) == int(g["stream_num_frames"]) == (T + fsf - 1) // fsf == g["offline_loglikes"].shape[0]
        assert np.isfinite(g["input"]).all() and np.isfinite(g["offline_loglikes"]).all()
    for p in rc.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stem in rc.CASES and p.stat().st_size < (1 << 20)


def test_the_table_covers_every_transform_size():
    """256, 512, 1024 and 2048 points; even and odd windows; an odd shift; a window as long as its transform."""
    geo = {n: rc.geometry(n) for n in rc.CASES}
    assert geo["r8k_iv"] == (200, 80, 256) and geo["r8k_win32"] == (256, 80, 256) and geo["r8k_win20"] == (160, 80, 256)
    assert geo["r8k_win33"] == (264, 80, 512) and geo["r11k"] == (275, 110, 512)
    assert geo["r22k"] == (551, 220, 1024) and geo["r32k_fbank"] == (800, 320, 1024)
    assert geo["r44k"] == (1102, 441, 2048) and geo["r48k"] == (1200, 480, 2048)
    assert {g[2] for g in geo.values()} == {256, 512, 1024, 2048}


@pytest.mark.parametrize("name", rc.DECODED)
def test_oracle_matches_reference_offline(oracles, name):
    g = rc.load_golden(name)
    orc, pcm = oracles(name)
    assert orc.mfcc.padded == rc.geometry(name)[2] and orc.mfcc.o.samp_freq == rc.rate(name)
    tr = orc.transcribe(pcm, nbest=rc.NBEST)
    assert tr.num_frames == int(g["offline_num_frames"])
    fd = np.abs(tr.feats - g["input"])
    print(f"{name}: rows up to {np.abs(g['input']).max():.4g}, max abs diff {fd.max():.3g}, 99 % below {np.quantile(fd, 0.99):.3g}")
    assert fd.max() < 2e-4 and np.quantile(fd, 0.99) < 1e-4
    assert int(g["rand_calls"]) == orc.rand_calls
    if "offline_ivector" in g.files:
        assert np.abs(tr.ivector - g["offline_ivector"][0]).max() < 1e-4
    ld = float(np.abs(tr.loglikes - g["offline_loglikes"]).max())
    print(f"{name}: log-likelihood max abs diff {ld:.3g}")
    assert ld < 1e-4
    assert [p.words for p in tr.nbest] == parse_nbest(bytes(g["offline_nbest_text"]))
    np.testing.assert_allclose([p.graph_cost for p in tr.nbest], g["offline_graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose([p.acoustic_cost for p in tr.nbest], g["offline_acoustic_cost"], rtol=2e-4, atol=2e-3)
    assert tr.text().split() == bytes(g["offline_nbest_text"]).split()


@pytest.mark.parametrize("name", rc.DECODED)
def test_oracle_matches_reference_streamed(oracles, name):
    """online2-cli-nnet3-decode-faster --samp-freq=<rate>: 5-best text, costs and frame count (there are no per-tick dumps at these
    rates: tests/gen_rate_golden.py)."""
    g = rc.load_golden(name)
    orc, pcm = oracles(name)
    tr = orc.transcribe_stream(pcm, nbest=rc.NBEST)
    assert tr.num_frames == int(g["stream_num_frames"])
    assert tr.text() == bytes(g["stream_nbest_text"])
    np.testing.assert_allclose([p.graph_cost for p in tr.nbest], g["stream_graph_cost"], rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose([p.acoustic_cost for p in tr.nbest], g["stream_acoustic_cost"], rtol=2e-4, atol=2e-3)


def test_oracle_fails_on_the_clip_without_a_frame(oracles):
    orc, pcm = oracles(rc.NO_FRAME)
    assert len(pcm) == rc.geometry(rc.NO_FRAME)[0] - 1
    for fn in (orc.transcribe, orc.transcribe_stream):
        with pytest.raises(RuntimeError, match="decoded no frames"):
            fn(pcm)


# ---------------------------------------------------------------------------------------------- the host side of the library
@pytest.mark.parametrize("name", list(rc.CASES))
def test_model_loads_and_describes_its_window(built, name):
    """The parent refused the 256- and 1024-point cases at load ("padded window size 256 unsupported by the HIP FFT (need 512 or 2048)")."""
    from rhasspy_speech_amd import _lib
    md, gd, _, _ = built(name)
    model = _lib.Model(md, gd)
    win, shift, padded = rc.geometry(name)
    kind = "fbank" if rc.CASES[name]["spec"].get("feature_type") == "fbank" else "mfcc"
    assert model.describe().startswith(f"{kind}: win={win} shift={shift} padded={padded} "), model.describe()[:120]
    assert model.sample_rate == float(rc.rate(name))


def _model_with_window(tmp_path, sample_frequency, frame_length, **spec):
    from rhasspy_speech_amd import synth
    from tests import cases
    s = dict(sample_frequency=sample_frequency, frame_length=frame_length, ivector_dim=0)
    s.update(spec)
    md, gd, _, _ = cases.build_case_files(dict(spec=s, graph="grammar", audio="zeros:0"), tmp_path)
    return md, gd


@pytest.mark.parametrize("sample_frequency, frame_length, padded", [(8000, 16.0, 128), (8000, 8.0, 64), (48000, 50.0, 4096), (16000, 300.0, 8192)])
def test_other_transform_sizes_are_still_refused_by_name(tmp_path, sample_frequency, frame_length, padded):
    from rhasspy_speech_amd import _lib
    md, gd = _model_with_window(tmp_path, sample_frequency, frame_length, low_freq=40, high_freq=-200)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert f"mfcc: padded window size {padded} unsupported by the HIP FFT (need 256, 512, 1024 or 2048)" in str(ei.value)


def test_a_16_khz_model_says_16000(tmp_path):
    from rhasspy_speech_amd import _lib
    from tests import cases
    md, gd, _, _ = cases.build_case_files(cases.CASES["tiny_u3_short"], tmp_path)
    assert _lib.Model(md, gd).sample_rate == 16000.0


def test_sample_rate_mismatch_message(built):
    """Kaldi's words (feat/online-feature.cc:86-101), with the model's rate in them; the stream transcriber checks its samp_freq -- the
    binary's --samp-freq, 16000 unless given -- before it opens a stream."""
    from rhasspy_speech_amd import _lib
    from rhasspy_speech_amd.transcribe_stream import KaldiNnet3StreamTranscriber
    md, gd, _, _ = built("r8k_iv")
    model = _lib.Model(md, gd)
    model.check_sample_rate(8000)
    with pytest.raises(_lib.RsError, match="Sampling frequency mismatch, expected 8000, got 16000"):
        model.check_sample_rate(16000.0)
    tr = KaldiNnet3StreamTranscriber(md, gd)
    assert tr.samp_freq == 16000.0
    with pytest.raises(RuntimeError, match="Sampling frequency mismatch, expected 8000, got 16000"):
        tr._open_stream(tr._ensure_loaded())
    ok = KaldiNnet3StreamTranscriber(md, gd, samp_freq=8000)
    assert ok._ensure_loaded().sample_rate == 8000.0 and ok._rate_error is None
    md22 = built("r22k")[0]
    with pytest.raises(_lib.RsError, match="Sampling frequency mismatch, expected 22050, got 8000"):
        _lib.Model(md22, built("r22k")[1]).check_sample_rate(8000)


def test_stream_shim_reads_samp_freq(built, capsys, monkeypatch):
    """--samp-freq on online2-cli-nnet3-decode-faster's command line (online2-cli-nnet3-decode-faster.cc:67-70); the wav binary has no
    such option.  Without it the stream binary assumes 16000 and an 8 kHz model ends it with Kaldi's message before it reads stdin."""
    import io
    import sys
    from rhasspy_speech_amd import kaldi_cli
    opts, config, pos = kaldi_cli.parse_command_line(["--samp-freq=8000", "--config=c", "--beam=12", "a", "b"])
    assert opts == {"samp_freq": 8000.0, "beam": 12.0} and config == "c" and pos == ["a", "b"]
    assert kaldi_cli.parse_command_line(["--config=c", "--samp-freq=22050.0"])[0] == {"samp_freq": 22050.0}
    with pytest.raises(ValueError, match="Invalid floating-point option"):
        kaldi_cli.parse_command_line(["--config=c", "--samp-freq=fast"])
    md, gd, wav, _ = built("r8k_iv")
    conf, mdl = md / "model" / "online" / "conf" / "online.conf", md / "model" / "model" / "final.mdl"
    with pytest.raises(ValueError, match="invalid option --samp-freq"):
        kaldi_cli.wav_main([f"--config={conf}", "--samp-freq=8000", str(mdl), str(gd / "HCLG.fst"), "ark:echo utt utt|", f"scp:echo utt {wav}|", "ark:-"])

    class _Stdin:
        buffer = io.BytesIO(b"\0" * 4096)
    monkeypatch.setattr(sys, "stdin", _Stdin)
    for extra in ([], ["--samp-freq=16000"], ["--samp-freq=44100"]):
        status = kaldi_cli.run(kaldi_cli.cli_main, [f"--config={conf}", *extra, str(mdl), str(gd / "HCLG.fst"), str(gd / "words.txt"), "ark:-"])
        got = extra[0].split("=")[1] if extra else "16000"
        assert status == 1 and f"Sampling frequency mismatch, expected 8000, got {got}" in capsys.readouterr().err
        assert _Stdin.buffer.tell() == 0      # (nothing was read)


def test_synth_defaults_write_the_bytes_they_always_wrote(tmp_path):
    """The new ModelSpec fields at their defaults, and spelled out, change no file of a 16 kHz model (the recorded hashes are those of
    tests/test_fbank_cpu.py, taken before either change); at another rate only the configuration differs."""
    from rhasspy_speech_amd import synth
    from tests.test_fbank_cpu import TINY_MODEL_SHA256

    def hashes(tag, **kw):
        synth.write_model_dir(tmp_path / tag, synth.tiny_spec(**kw))
        return {str(f.relative_to(tmp_path / tag)): hashlib.sha256(f.read_bytes().replace(str(tmp_path / tag).encode(), b"<ROOT>/m")).hexdigest()
                for f in sorted((tmp_path / tag).rglob("*")) if f.is_file()}

    assert hashes("a") == TINY_MODEL_SHA256
    assert hashes("b", sample_frequency=16000, low_freq=20, high_freq=-400, mfcc_defaults=False) == TINY_MODEL_SHA256
    r8 = hashes("c", sample_frequency=8000, low_freq=40, high_freq=-200)
    assert {k for k in r8 if r8[k] != TINY_MODEL_SHA256[k]} == {"model/online/conf/mfcc.conf"}
    assert (tmp_path / "c" / "model" / "online" / "conf" / "mfcc.conf").read_text() == (
        "# hires MFCC (egs/wsj/s5/conf/mfcc_hires.conf)\n--use-energy=false\n--num-mel-bins=40\n--num-ceps=40\n--low-freq=40\n--high-freq=-200\n"
        "--sample-frequency=8000\n")
    # the filterbank writer's lines, and the configuration of r8k_default
    synth.write_model_dir(tmp_path / "d", synth.tiny_spec(feature_type="fbank"))
    assert (tmp_path / "d" / "model" / "online" / "conf" / "fbank.conf").read_text() == "--num-mel-bins=40\n--low-freq=20\n--high-freq=-400\n--sample-frequency=16000\n"
    synth.write_model_dir(tmp_path / "e", synth.tiny_spec(**rc.CASES["r8k_default"]["spec"]))
    assert (tmp_path / "e" / "model" / "online" / "conf" / "mfcc.conf").read_text() == "--sample-frequency=8000\n--use-energy=false\n"
    with pytest.raises(ValueError):
        synth.write_model_dir(tmp_path / "f", synth.tiny_spec(mfcc_defaults=True))
