"""FbankKernel beside MfccKernel on the headline batch geometry (256 x 3 s, the zamia-like-S model): the feature stage of
un-overlapped decode calls on samples resident in HBM (rs_result_timings, device events: the stage is the one feature launch), the
two models taken in turn.  The filterbank model is the same spec with feature_type="fbank": 40 bins in place of 40 cepstra from 40
bins, so the kernel is MfccKernel's front end and mel products without the DCT.  Needs the GPU.
  usage: python profiles/micro/fbank_kernel_time.py [rounds, default 5]"""
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from rhasspy_speech_amd import _lib, synth  # noqa: E402
from tests import configs  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
if not torch.cuda.is_available():
    raise SystemExit("fbank_kernel_time.py needs an MI355X")
pcms = configs.grammar_utterances(256, 0)
d_pcm = torch.from_numpy(np.concatenate(pcms)).to("cuda:0")
offsets = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
with tempfile.TemporaryDirectory(prefix="rs_fbank_time_") as td:
    models = {}
    for kind in ("mfcc", "fbank"):
        spec = synth.ModelSpec(feature_type=kind)
        synth.write_model_dir(Path(td) / kind / "model", spec)
        synth.make_grammar_graph(Path(td) / kind / "graph", spec, seed=11)
        models[kind] = _lib.Model(Path(td) / kind / "model", Path(td) / kind / "graph", _lib.default_opts(device_id=0))
        models[kind].to_device()
        for _ in range(2):      # warm-up: code objects, arenas, the dither table
            models[kind].decode_batch_device(d_pcm.data_ptr(), offsets)
    ms = {k: [] for k in models}
    for _ in range(rounds):
        for kind, model in models.items():
            ms[kind].append(float(model.decode_batch_device(d_pcm.data_ptr(), offsets).timings()[1]))
    for kind, v in ms.items():
        print(f"{kind}: feature stage of 256 x 3 s, {rounds} calls: min {min(v) * 1e3:.0f} us, median {sorted(v)[len(v) // 2] * 1e3:.0f} us  ({' '.join(f'{x * 1e3:.0f}' for x in v)})")
