"""Log-mel filterbank models (--feature-type=fbank) without a GPU: the configuration reader and table builder (model.cc) through the
library and through a stand-alone host program under the address and undefined-behaviour sanitizers, the synthetic model writer, and
the goldens of tests/fbank_cases.py."""
import hashlib
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import fbank_cases as fc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (model_dir, graph_dir, wav, pcm), each case's files written once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = fc.build_case_files(name, tmp_path_factory.mktemp(name))
        return done[name]
    return get


def _conf(model_dir, name):
    return model_dir / "model" / "online" / "conf" / name


def test_fbank_model_loads_and_only_the_missing_device_stops_it(built):
    """The parent refused the directory at load ("feature type fbank is not supported by the HIP path").  Now it loads on the host,
    says what it read, and without a GPU a decode fails the way every model's does: no device, no fall-back."""
    import torch
    from rhasspy_speech_amd import _lib
    md, gd, _, pcm = built("fb40_iv")
    model = _lib.Model(md, gd)
    text = model.describe()
    assert "fbank: win=400 shift=160 padded=512 mel_bins=40 dim=40 use_energy=0 htk_compat=0 use_log=1 use_power=1 dither=1\n" in text
    assert "mfcc:" not in text and "nnet: input_dim=40 " in text
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RsError) as ei:
            model.decode_batch([pcm])
        assert ei.value.status == _lib.RS_ERR_DEVICE and "no CPU fallback" in str(ei.value)
        assert "feature type" not in str(ei.value) and "option" not in str(ei.value)


def test_mfcc_model_describes_itself_as_before(tmp_path):
    from rhasspy_speech_amd import _lib, synth
    spec = synth.tiny_spec()
    synth.write_model_dir(tmp_path / "model", spec)
    synth.make_grammar_graph(tmp_path / "graph", spec)
    text = _lib.Model(tmp_path / "model", tmp_path / "graph").describe()
    assert text.startswith("mfcc: win=400 shift=160 padded=512 mel_bins=40 ceps=40 dither=1\nnnet_input_cmvn: 0\n") and "fbank" not in text


def _copy(built, name, tmp_path):
    """A private copy of the case's model directory (the configuration files name each other by absolute path: rewritten)."""
    md, gd, _, _ = built(name)
    dst = tmp_path / "model"
    shutil.copytree(md, dst)
    for f in (dst / "model" / "online" / "conf").iterdir():
        f.write_text(f.read_text().replace(str(md), str(dst)))
    return dst, gd


def _append(path, line):
    path.write_text(path.read_text() + line + "\n")


@pytest.mark.parametrize("case, file, line, needle", [
    ("fb40_iv", "fbank.conf", "--cepstral-lifter=22", "Invalid option --cepstral-lifter=22"),      # an MFCC option is not a filterbank option
    ("fb40_iv", "fbank.conf", "--htk-mode=true", "Invalid option --htk-mode=true"),                # (the reference does not register it either)
    ("fb40_iv", "online.conf", "--feature-type=plp", "feature type plp is not supported by the HIP path (supported: mfcc, fbank)"),
    ("fb40_iv", "online.conf", "--feature-type=nonsense", "Invalid feature type: nonsense. Supported feature types: mfcc, plp, fbank."),
    ("fb40_iv", "fbank.conf", "--num-mel-bins=200", "You may have set --num-mel-bins too large."),
    ("fb40_win100", "fbank.conf", "--num-mel-bins=200", "are more than the 128 the HIP path supports"),      # (fits the 2048-point FFT, not the row)
    ("fb80_noiv", "fbank.conf", "--use-energy=true", "Input feature dimension mismatch: got 81 but network expects 80"),
    ("fb40_iv", "fbank.conf", "--use-energy=true", "iVector extractor: global CMVN stats dim 40 != feature dim 41"),
    ("fb40_nnetcmvn", "fbank.conf", "--num-mel-bins=39", "global cmvn stats have the wrong dimension"),
    ("fb40_iv", "fbank.conf", "--vtln-low=200", "--vtln-low=200 is not supported"),
    ("fb40_iv", "fbank.conf", "--debug-mel=true", "--debug-mel=true is not supported"),
    ("fb40_iv", "fbank.conf", "--snip-edges=false", "fbank: --snip-edges=false is not supported"),
])
def test_configuration_errors(built, tmp_path, case, file, line, needle):
    """What the reference refuses is refused in its words; what only this path cannot do is refused loudly, never dropped or truncated."""
    from rhasspy_speech_amd import _lib
    md, gd = _copy(built, case, tmp_path)
    _append(_conf(md, file), line)
    with pytest.raises(_lib.RsError) as ei:
        _lib.Model(md, gd)
    assert needle in str(ei.value), str(ei.value)


def test_only_the_selected_types_config_counts(built, tmp_path):
    """online-nnet2-feature-pipeline.cc:36-55: an --mfcc-config beside --feature-type=fbank is read and ignored (13 cepstra would not
    fit this network); default --vtln-* values and --debug-mel=false are not errors."""
    from rhasspy_speech_amd import _lib
    md, gd = _copy(built, "fb40_iv", tmp_path)
    _conf(md, "mfcc.conf").write_text("--num-ceps=13\n--use-energy=true\n")
    _append(_conf(md, "online.conf"), f"--mfcc-config={_conf(md, 'mfcc.conf')}")
    _append(_conf(md, "fbank.conf"), "--vtln-low=100\n--vtln-high=-500\n--debug-mel=false")
    assert "fbank: win=400 shift=160 padded=512 mel_bins=40 dim=40 " in _lib.Model(md, gd).describe()
    _conf(md, "mfcc.conf").write_text("--no-such-option=1\n")      # read all the same
    with pytest.raises(_lib.RsError, match="Invalid option --no-such-option=1"):
        _lib.Model(md, gd)


# sha256 of every file synth.write_model_dir(tiny_spec()) wrote on the commit before the filterbank fields were added to ModelSpec (the
# directory's own path, which the configuration files carry, replaced by <ROOT>): the existing goldens depend on these bytes
TINY_MODEL_SHA256 = {
    "model/model/final.mdl": "f3cd52d4ed52dc3e12ea4f5c597431b45e95623a5878a1f3cfea2710429f9fbf",
    "model/model/tree": "6cac224fd09fe31a449fcff82af2ad386da8a9f90a6503009eb9836cf218e150",
    "model/online/conf/ivector_extractor.conf": "6860903944fa876333e194f0195b5a5561e646559ce5a6c85dfc020dc3d43cc0",
    "model/online/conf/mfcc.conf": "f161107776f49c13124b47872d2d6f23bc61ae900194a51375119390c553d84f",
    "model/online/conf/online.conf": "82e310120116c38e2d2a4ea8dcdbf876166c093b369aea2d74f3c26c773845fb",
    "model/online/conf/online_cmvn.conf": "a2f3571754b64297cb7efb2e7ca3df61995c5a45fcbb97188f90613552bb2dfe",
    "model/online/conf/splice.conf": "9f0c5f7c82d18eaf25d8bce470efa9f7741f88411fe428774bc0a9bb69a24756",
    "model/online/ivector_extractor/final.dubm": "b8dc00f2c949241d531b2d93acc9aff8a2c88619cd5c0a01a37c4ac4d7dc03ee",
    "model/online/ivector_extractor/final.ie": "374af1c8cdb2ce82b004a2bb0bc6fcd001a1772c6a45460ba378d3078eda31d5",
    "model/online/ivector_extractor/final.mat": "ad6d4702b67b83dddad471a68e64e2e585704373c6f1e85107331dd39e32915a",
    "model/online/ivector_extractor/global_cmvn.stats": "2749939af543546999854b481b3b396e9bbb868e873f6e6214c1f51de462df11",
}


def test_default_model_spec_writes_the_bytes_it_always_wrote(tmp_path):
    from rhasspy_speech_amd import synth
    synth.write_model_dir(tmp_path / "m", synth.tiny_spec())
    got = {str(f.relative_to(tmp_path / "m")): hashlib.sha256(f.read_bytes().replace(str(tmp_path).encode(), b"<ROOT>")).hexdigest()
           for f in sorted((tmp_path / "m").rglob("*")) if f.is_file()}
    assert got == TINY_MODEL_SHA256


def test_fbank_model_spec_sizes_everything_from_the_row(built):
    """conf/fbank.conf and the --feature-type / --fbank-config lines; network input, extractor LDA and global_cmvn.stats as wide as the row."""
    from rhasspy_speech_amd import synth
    for name in fc.CASES:
        dim, bins, _ = fc.expected_layout(name)
        spec = synth.tiny_spec(**fc.CASES[name]["spec"])
        assert spec.feat_dim == dim
        md = built(name)[0]
        online = _conf(md, "online.conf").read_text()
        assert "--feature-type=fbank\n" in online and "mfcc" not in online and not _conf(md, "mfcc.conf").exists()
        if spec.fbank_config:
            assert f"--fbank-config={_conf(md, 'fbank.conf')}\n" in online and f"--num-mel-bins={bins}\n" in _conf(md, "fbank.conf").read_text()
        else:
            assert "fbank-config" not in online and not _conf(md, "fbank.conf").exists()
    with pytest.raises(ValueError):
        synth.tiny_spec(feature_type="plp").feat_dim


def test_goldens_are_there_for_every_case():
    for name, case in fc.CASES.items():
        g = fc.load_golden(name)
        assert bytes(g["case_json"]).decode() == __import__("json").dumps(case, sort_keys=True), name      # (made from this table)
        if name == "fb40_len0":
            assert int(g["offline_status"]) != 0 and int(g["stream_status"]) != 0
            assert b"decoded no frames" in bytes(g["offline_stderr"]) and b"decoded no frames" in bytes(g["stream_stderr"])
            continue
        dim = fc.expected_layout(name)[0]
        keys = {"input", "rand_calls"} | {f"{m}_{k}" for m in ("offline", "stream")
                                          for k in ("status", "nbest_text", "graph_cost", "acoustic_cost", "num_frames", "loglikes")}
        if case["spec"].get("ivector_dim", 1) > 0:
            keys |= {"offline_ivector", "offline_chunk_tick", "stream_ivector", "stream_chunk_tick"}
        assert keys <= set(g.files), (name, keys - set(g.files))
        assert int(g["offline_status"]) == 0 and int(g["stream_status"]) == 0
        assert g["input"].shape[1] == dim and g["offline_loglikes"].shape == (int(g["offline_num_frames"]), 48 if name != "fb40_arpa" else 80)
        assert g["stream_loglikes"].shape == g["offline_loglikes"].shape
        assert len(g["offline_graph_cost"]) == len(g["offline_acoustic_cost"]) >= 1
        for k in ("input", "offline_loglikes", "stream_loglikes"):
            assert np.isfinite(g[k]).all()
        if name in fc.LINEAR:
            assert np.abs(g["offline_loglikes"]).max() < 1e4 and np.abs(g["stream_loglikes"]).max() < 1e4
    assert fc.load_golden("fb40_winenergy_floor")["input"][:, 0].tolist() == [0.0] * 98      # log(energy-floor = 1) on every frame
    for p in fc.GOLDEN.iterdir():
        assert p.suffix == ".npz" and p.stem in fc.CASES and p.stat().st_size < (1 << 20)


def test_config_reader_and_table_builder_under_sanitizers(built, tmp_path):
    """tests/host/fbank_conf_check.cc (its own main; address + undefined-behaviour sanitizers) reads every case's fbank.conf, builds
    the tables and walks them as the kernel does; the row layout it prints is the case table's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "fbank_conf_check"
    # (model.cc is the library's largest host file: the three sources are compiled side by side without optimisation, and the
    # linker drops the model reader's sections, which would ask for the rest of the library)
    flags = [cxx, "-std=c++17", "-g1", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffunction-sections", "-fdata-sections"]
    srcs = [ROOT / "tests" / "host" / "fbank_conf_check.cc", CSRC / "model.cc", CSRC / "kaldi_io.cc"]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    jobs = [subprocess.Popen(flags + ["-c", str(s), "-o", str(o)]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0, 0, 0]
    subprocess.run(flags + ["-Wl,--gc-sections", *map(str, objs), "-o", str(exe)], check=True)
    args = []
    for name in fc.CASES:
        conf = _conf(built(name)[0], "fbank.conf")
        args += [name, str(conf) if conf.exists() else "-"]
    bad = tmp_path / "bad.conf"
    bad.write_text("--num-mel-bins=40\n--num-ceps=13\n")
    two = tmp_path / "two.conf"
    two.write_text("--num-mel-bins=2\n")
    p = subprocess.run([str(exe), *args, "unknown_key", str(bad), "two_bins", str(two)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(fc.CASES) + 2
    for name, line in zip(fc.CASES, lines):
        dim, bins, ecol = fc.expected_layout(name)
        padded = 2048 if fc.CASES[name]["spec"].get("frame_length") == 100.0 else 512
        head = f"{name} dim={dim} bins={bins} energy_col={ecol} mel_col0={1 if ecol == 0 else 0} padded={padded} weights="
        assert line.startswith(head) and int(line[len(head):]) >= bins, line
    assert lines[-2] == f"unknown_key error: Invalid option --num-ceps=13 in config file {bad}"
    assert lines[-1] == "two_bins error: Must have at least 3 mel bins"
