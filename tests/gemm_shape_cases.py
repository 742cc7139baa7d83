"""A family of small networks, switch settings and clip lengths that puts a layer GEMM on every kernel instantiation the launch
policy (csrc/gemm_launch.cc) can plan, shared by tests/test_gemm_shapes_cpu.py and tests/test_gpu_gemm_shapes.py.

A row of CASES names a net (NETS: synth.ModelSpec keyword arguments; 16 Gaussians, few phones: the load is short), options, the
RS_GEMM_* environment, clip lengths in samples (0: an utterance without a frame) and, per op the row is about, the `gemm_launch:`
lines rs_model_describe must show after one batch call with keep_intermediates=1.  RS_GEMM_CUS shrinks the device the planner sees
(8 CUs: 16 slots of two workgroups per CU), so every branch of the policy turns over at a few hundred to a few thousand rows.

What a line is made of is restated here from the sources, independently of the library, so that the CPU test can hand the real
planner (tests/host/gemm_launch_check.cc, descriptor mode) the descriptor the model will build on the GPU:
  * net_ops(): the ops synth.build_nnet's config compiles to (one GEMM per affine / TDNN / linear component, the element-wise
    components behind it folded in as stages, a Sum(Scale(0.66, prev), .) folded in as a residual) -- held to the `op:` lines of
    rs_model_describe on a CPU-loaded model by the CPU test;
  * extents(): the frames of context every op's output is read with, hence (PlanRowLists, csrc/call_plan.cc) the rows the op is
    evaluated on -- all rows, a trimmed row list, the frames only, every fsf-th frame -- and the span of 128 / 160 list rows;
  * classify(): which buffers carry an operand image, which are (also) stored as floats (Model::ToDevice, Model::MakeGemm).
The GPU test sees the same lines come out of the model, rows and k-steps included: a restatement that drifts from the library
fails there, one that drifts from the planner fails on the CPU.

UNREACHABLE lists the instantiations of the dispatchers no model reaches in the shipped build, with the rule that excludes each."""
from __future__ import annotations

import re
from pathlib import Path
from typing import Dict, List, Optional, Tuple

from rhasspy_speech_amd import synth

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "rhasspy_speech_amd" / "csrc"
LDA_OP = "ivector.splice+lda (one run)"
DEVICE_CUS = 256          # MI355X; every case sets RS_GEMM_CUS, so the figure only matters to the baseline launches

SMALL = dict(ivector_dim=10, num_gauss=16, lda_dim=12, num_phones=24, dither=0.0)
NETS: Dict[str, dict] = {
    # first layer 250 (40 + 40 + 40 + 10 wide float segments: GemmKernelB3) -> 250 x 3 at -1,0,1 -> 250 x 3 at -3,0,3 (both
    # strip-eligible) -> prefinal 250 -> 362 pdfs (two column tiles, the second mostly padding)
    "t250": dict(SMALL, hidden_dim=250, prefinal_dim=250, num_phones=181, layer_offsets=((0,), (-1, 0, 1), (-3, 0, 3))),
    # no column padding at all: 256 everywhere, 256 pdfs
    "t256": dict(SMALL, hidden_dim=256, prefinal_dim=256, num_phones=128, layer_offsets=((0,), (-1, 0, 1), (-3, 0, 3)), seed=3),
    # the 256 x 128 narrow tile: 128-wide hidden layers, a 96-wide prefinal layer, 130 pdfs (one tile of >= 96 columns)
    "t128": dict(SMALL, hidden_dim=128, prefinal_dim=96, num_phones=65, layer_offsets=((0,), (-1, 0, 1), (-3, 0, 3)), seed=4),
    # segment widths that are no multiple of the k-step: 100-wide hidden layers (7 k-steps per segment, the last with 4 live columns)
    "t100": dict(SMALL, hidden_dim=100, prefinal_dim=250, num_phones=50, layer_offsets=((0,), (-1, 0, 1), (-2, 0, 2)), seed=5),
    # offsets 80 rows apart: three interleaved segments that are NOT strip-eligible (far_offsets of the host check)
    "tfar": dict(SMALL, hidden_dim=250, prefinal_dim=250, num_phones=40, layer_offsets=((0,), (-40, 0, 40)), seed=6),
    # a strip-eligible layer (+-3) whose output only the frames read, in a net with 33 frames of context: between two utterances its
    # row list skips 66 halo rows, so 128 list rows of short utterances reach over more rows than the strip holds (map_wide of the
    # host check); one long utterance fits (map_fits)
    "twide": dict(SMALL, hidden_dim=250, prefinal_dim=250, num_phones=40, layer_offsets=((0,), (-30, 0, 30), (-3, 0, 3)), seed=13),
    # the exact-FP32 kernels: 65-wide hidden layers (first width above the four-wave tile), prefinal 64, 40 pdfs; no split weights below 96
    "x65": dict(SMALL, hidden_dim=65, prefinal_dim=64, num_phones=20, layer_offsets=((0,), (-1, 0, 1)), seed=7),
    # ... and widths the 45 % padding rule sends there: 270 (47 % of 512) and 328
    "x270": dict(SMALL, hidden_dim=270, prefinal_dim=328, num_phones=40, layer_offsets=((0,), (-1, 0, 1)), seed=8),
    # a factorised net: bare 128-wide linear bottlenecks (no stage), two-segment affines, folded residuals 0.66 * previous layer
    "f256": dict(SMALL, tdnnf=True, hidden_dim=256, bottleneck_dim=128, prefinal_dim=256, num_phones=64,
                 layer_offsets=((0,), (-1, 0, 1), (-3, 0, 3), (-3, 0, 3)), seed=9),
    # KSteps at the 32 PlanB3J asks of the 160-row tile (two segments of a 256-wide bottleneck) and just under it (240: 30)
    "f256_k32": dict(SMALL, tdnnf=True, hidden_dim=256, bottleneck_dim=256, prefinal_dim=256, num_phones=64,
                     layer_offsets=((0,), (-3, 0, 3)), seed=10),
    "f256_k30": dict(SMALL, tdnnf=True, hidden_dim=256, bottleneck_dim=240, prefinal_dim=256, num_phones=64,
                     layer_offsets=((0,), (-3, 0, 3)), seed=11),
    # without an iVector: the first layer is three 40-wide float segments and nothing per utterance (n = 120)
    "t250_noiv": dict(SMALL, ivector_dim=0, hidden_dim=250, prefinal_dim=250, num_phones=125, layer_offsets=((0,), (-1, 0, 1), (-3, 0, 3)), seed=12),
}

# Instantiations of the four dispatch switches that no model reaches in the shipped build (the label as DescribeGemmLaunch prints it,
# then the rule of gemm_launch.cc that excludes it).  A -DRS_TUNING build reaches them; the suite does not build one.
UNREACHABLE: Dict[str, str] = {
    **{f"Exact<{s},0,0>": "PlanExact: vec = Aligned16(d); every frame buffer's row pitch is RoundUp(dim, 4) floats, every segment starts at column 0 "
                          "and arena blocks are 256-byte aligned, so no descriptor of a model misaligns a source (the host check's src_misaligned does)"
       for s in ("1,4,1", "2,4,1", "4,2,2", "3,2,2", "2,2,2")},
    **{f"Exact<{s},1,0>": "PlanExact: dma = vec && sw.dma; RS_GEMM_DMA is a TuneEnv switch (1 unless the build has -DRS_TUNING)"
       for s in ("1,4,1", "2,4,1", "4,2,2", "3,2,2", "2,2,2")},
    "Exact<2,4,1,1,1>": "PlanExact, n <= 64: cost(64, 64) = r64 * 64 * 64 * 0.97 with r64 <= 2 * r128 rounds is always below cost(128, 64) = r128 * 128 * 64: "
                        "the 128-row four-wave tile needs RS_GEMM_NARROW_BM=128 (TuneEnv)",
    "Exact<4,2,2,1,1>": "PlanExact, n > 64: c64 = r64 * 64 * 0.97 <= r128 * 124.2 < c128 = r128 * 128 for every row count: the 128-row tile needs RS_GEMM_BM=128 (TuneEnv)",
    "B3I<1,0,4>": "PlanB3I: kps of the 32-row tile is sw.b3i_kps, 8 unless RS_GEMM_B3I_KPS (TuneEnv) says 4",
    "B3I<1,0,2>": "PlanB3I: kps of the 32-row tile is 2 only for an RS_GEMM_B3I_KPS (TuneEnv) other than 4 or 8",
}
# (the alternating block order, a negative nfirst, is no instantiation of its own: RS_GEMM_B3J_STAGGER=2 (TuneEnv) asks for it, the
# host check's coverage sweep walks it)


# ---------------------------------------------------------------------------------------------- the net, restated
def spec_of(net: str) -> synth.ModelSpec:
    return synth.ModelSpec(**NETS[net])


def net_ops(spec: synth.ModelSpec) -> List[dict]:
    """The GEMM ops of synth.build_nnet(spec) in order: name, n, segs [(source, row offset, columns)] ("input", "ivector" or the
    producing op), res (source of a folded 0.66 residual or None), stages (element-wise components folded in)."""
    C, D, H = spec.num_ceps, spec.ivector_dim, spec.hidden_dim
    assert spec.layer_offsets[0] == (0,)      # the fixed lda transform is composed with the first layer's affine: one GEMM on the inputs
    ops = [dict(name="tdnn1.affine+tdnn1.relu+tdnn1.batchnorm", n=H, segs=[("input", o, C) for o in spec.lda_offsets] + ([("ivector", 0, D)] if D else []),
                res=None, stages=2)]
    prev, prev_dim = ops[0]["name"], H
    for li, offs in enumerate(spec.layer_offsets[1:], start=2):
        if spec.tdnnf:
            lo, ro, B = [o for o in offs if o <= 0], [o for o in offs if o >= 0], spec.bottleneck_dim
            lin = f"tdnnf{li}.linear"
            ops.append(dict(name=lin, n=B, segs=[(prev, o, prev_dim) for o in lo], res=None, stages=0))
            ops.append(dict(name="+".join(f"tdnnf{li}.{c}" for c in ("affine", "relu", "batchnorm", "dropout", "noop")), n=H, segs=[(lin, o, B) for o in ro],
                            res=prev if prev_dim == H else None, stages=2))
        else:
            ops.append(dict(name=f"tdnn{li}.affine+tdnn{li}.relu+tdnn{li}.batchnorm", n=H, segs=[(prev, o, prev_dim) for o in offs], res=None, stages=2))
        prev, prev_dim = ops[-1]["name"], H
    ops.append(dict(name="prefinal-chain.affine+prefinal-chain.relu+prefinal-chain.batchnorm", n=spec.prefinal_dim, segs=[(prev, 0, prev_dim)], res=None, stages=2))
    ops.append(dict(name="output.affine+output", n=spec.num_pdfs, segs=[(ops[-1]["name"], 0, spec.prefinal_dim)], res=None, stages=0))
    return ops


def short(name: str) -> str:
    """"tdnn2" for "tdnn2.affine+tdnn2.relu+tdnn2.batchnorm", "tdnnf3.linear", "tdnnf3.affine", "prefinal", "output": the keys of a row's `expect`."""
    if name.startswith("ivector."):
        return "ivector_lda"
    first = name.split("+")[0]
    return first if first.startswith("tdnnf") else first.split(".")[0].replace("prefinal-chain", "prefinal")


def extents(ops: List[dict], fsf: int = 1) -> Tuple[Dict[str, Tuple[int, int, int]], int, int]:
    """({buffer: (lext, rext, stride)}, L, R): the frames left and right of an utterance's own a buffer is read at, and fsf where all its
    readers are evaluated on every fsf-th frame and read it at offsets that are multiples of fsf."""
    ext = {o["name"]: [0, 0] for o in ops}
    ext["input"] = [0, 0]
    stride = {o["name"]: 1 for o in ops}
    stride[ops[-1]["name"]] = fsf
    readers: Dict[str, List[Tuple[str, int]]] = {}
    for o in reversed(ops):
        srcs = [(s, off) for s, off, _ in o["segs"] if s != "ivector"] + ([(o["res"], 0)] if o["res"] else [])
        for s, off in srcs:
            readers.setdefault(s, []).append((o["name"], off))
    for o in reversed(ops):
        name = o["name"]
        if name in readers:
            for r, off in readers[name]:
                ext[name][0] = max(ext[name][0], ext[r][0] - off)
                ext[name][1] = max(ext[name][1], ext[r][1] + off)
            stride[name] = fsf if all(stride[r] == fsf and off % fsf == 0 for r, off in readers[name]) else 1
    for r, off in readers["input"]:
        ext["input"][0] = max(ext["input"][0], ext[r][0] - off)
        ext["input"][1] = max(ext["input"][1], ext[r][1] + off)
    L, R = ext["input"]
    return {k: (v[0], v[1], stride.get(k, 1)) for k, v in ext.items()}, L, R


def num_frames(samples: int) -> int:
    """25 ms windows every 10 ms at 16 kHz, snip-edges."""
    return 0 if samples < 400 else 1 + (samples - 400) // 160


def _span_of_runs(runs: List[Tuple[int, int]], window: int) -> int:
    """call_plan.cc, SpanOfRuns: `window` consecutive entries of a list made of runs (first row, length) reach over at most this many rows."""
    worst, b, inner = 0, 0, 0
    for a in range(len(runs) - 1):
        if b <= a:
            b, inner = a + 1, 0
        while b + 1 < len(runs) and inner + runs[b][1] <= window - 2:
            inner += runs[b][1]
            b += 1
        worst = max(worst, runs[b][0] - (runs[a][0] + runs[a][1]) - inner)
        if b > a + 1:
            inner -= runs[a + 1][1]
    return window + worst


def op_rows(ext: Tuple[int, int, int], L: int, R: int, T: List[int]) -> dict:
    """rows / map / span128 / span160 of an op whose output has the extents `ext`, for a batch of utterances of T frames."""
    lext, rext, st = ext
    base = [0]
    for t in T:
        base.append(base[-1] + t + L + R)
    if st == 1 and lext >= L and rext >= R:
        return dict(rows=base[-1], map=0, span128=0, span160=0)
    if st > 1:
        return dict(rows=sum((t + rext - 1) // st + lext // st + 1 for t in T if t > 0), map=1, span128=0, span160=0)
    runs = [(base[u] + L - lext, t + lext + rext) for u, t in enumerate(T) if t > 0]
    return dict(rows=sum(n for _, n in runs), map=1, span128=_span_of_runs(runs, 128), span160=_span_of_runs(runs, 160))


def _padding_ok(n: int, narrow: bool) -> bool:
    n3 = (n + 255) // 256 * 256
    return (n3 == 256 and n >= 96 and narrow) or (n3 - n) * 100 <= n3 * 45


def classify(ops: List[dict], env: Dict[str, str]) -> Dict[str, dict]:
    """Per op the GemmDev fields that follow from the net and the switches: w3, w3i, interleave, the per-segment image flags, out_img,
    write_f32, res (0 none, 1 floats, 2 operand image)."""
    on = lambda k: env.get(k) is None or int(env[k]) != 0
    narrow, images_on = on("RS_GEMM_B3_NARROW"), on("RS_GEMM_B3") and on("RS_GEMM_B3I")
    image, f32 = {"input": False}, {"input": True, ops[-1]["name"]: True}
    plan = {}
    for o in ops:
        w3 = o["n"] >= 96 and _padding_ok(o["n"], narrow)
        frame_fed = all(s != "ivector" for s, _, _ in o["segs"])
        by_image = w3 and frame_fed and all(s != "input" for s, _, _ in o["segs"])
        for s, _, _ in o["segs"]:
            if s != "ivector":
                (image if by_image else f32)[s] = True
        res_by_image = by_image and on("RS_RESIDUAL_IMAGE")
        if o["res"]:
            (image if res_by_image else f32)[o["res"]] = True
        first = o["segs"][0]
        plan[o["name"]] = dict(w3=w3, w3i=w3 and frame_fed, by_image=res_by_image,
                               interleave=w3 and len(o["segs"]) > 1 and all(s == first[0] and n == first[2] for s, _, n in o["segs"]))
    out = {}
    for o in ops:
        p = plan[o["name"]]
        d = dict(w3=int(p["w3"] and on("RS_GEMM_B3")), w3i=int(p["w3i"] and images_on), interleave=int(p["interleave"]),
                 seg_img=[int(images_on and s != "ivector" and image.get(s, False)) for s, _, _ in o["segs"]],
                 out_img=int(images_on and image.get(o["name"], False)), write_f32=1,
                 res=0 if not o["res"] else (2 if images_on and p["by_image"] and p["w3i"] else 1))
        if d["out_img"]:
            d["write_f32"] = int(f32.get(o["name"], False))
        out[o["name"]] = d
    return out


def _writes_image(d: dict, o: dict, env: Dict[str, str]) -> bool:
    """GemmWritesImage: B3IUsable or B3Usable (sources are aligned in every model)."""
    return bool(d["w3"]) and _padding_ok(o["n"], env.get("RS_GEMM_B3_NARROW") is None or int(env["RS_GEMM_B3_NARROW"]) != 0)


def descriptors(case: dict) -> Dict[str, str]:
    """{op name: descriptor line for `gemm_launch_check <file>`} for the batch call of a case."""
    spec = spec_of(case["net"])
    ops, env = net_ops(spec), case.get("env", {})
    ext, L, R = extents(ops, case.get("opts", {}).get("frame_subsampling_factor", 1))
    if spec.ivector_dim:      # (the iVector branch's splice reaches over the input too)
        L, R = max(L, spec.splice_left), max(R, spec.splice_right)
    T = [num_frames(n) for n in case["clips"]]
    cls = classify(ops, env)
    switches = ",".join(f"{k[len('RS_GEMM_'):]}={v}" for k, v in env.items() if k.startswith("RS_GEMM_") and k != "RS_GEMM_B3_EXCLUSIVE") or "-"
    out = {}
    if spec.ivector_dim:      # splice + LDA of the iVector branch on every row of the call, as ONE run of 7 x 40 floats per row (pitch 40); both launches alike
        k = spec.num_ceps * (spec.splice_left + spec.splice_right + 1)
        out[LDA_OP] = (f"rows={sum(t + L + R for t in T)} cu={DEVICE_CUS} switches={switches} n={spec.lda_dim} w3=0 w3i=0 interleave=0 share=1 exclusive=0 write_f32=1 "
                       f"out_img=0 res=0 map=0 span128=0 span160=0 segs=0:{spec.num_ceps}:0:{k}:0:0:0 name={LDA_OP}")
    for o in ops:
        d, r = cls[o["name"]], op_rows(ext[o["name"]], L, R, T)
        if d["out_img"] and not _writes_image(d, o, env):
            d["write_f32"] = 1
        ld = lambda s, n: (n + 3) // 4 * 4
        segs = ";".join(f"{img}:{ld(s, n)}:0:{n}:{off}:{int(s == 'ivector')}:0" for (s, off, n), img in zip(o["segs"], d["seg_img"]))
        out[o["name"]] = (f"rows={r['rows']} cu={DEVICE_CUS} switches={switches} n={o['n']} w3={d['w3']} w3i={d['w3i']} interleave={d['interleave']} share=1 "
                          f"exclusive={int('RS_GEMM_B3_EXCLUSIVE' in env)} write_f32={d['write_f32']} out_img={d['out_img']} res={d['res']} map={r['map']} "
                          f"span128={r['span128']} span160={r['span160']} segs={segs} name={o['name']}")
    return out


# ---------------------------------------------------------------------------------------------- the dispatchers' labels
def dispatch_labels() -> List[str]:
    """Every instantiation the four dispatch switches can launch, as DescribeGemmLaunch names it, from the `case ...: return Launch...<...>`
    lines of the .hip files (template defaults filled in; the exact kernels times {scalar, vec, dma}: LaunchGemmT)."""
    labels = []
    pat = re.compile(r"^\s*case [^:]+: return (Launch\w+)<([^>]*)>\(", re.M)
    for fname, launcher in (("nnet_kernels.hip", "LaunchGemmT"), ("nnet_gemm_b3.hip", "LaunchB3"), ("nnet_gemm_b3i.hip", "LaunchB3I"), ("nnet_gemm_b3j.hip", "LaunchB3J")):
        found = [m.group(2) for m in pat.finditer((CSRC / fname).read_text()) if m.group(1) == launcher]
        assert found, fname
        for args in found:
            a = [{"true": "1", "false": "0"}.get(x.strip(), x.strip()) for x in args.split(",")]
            if launcher == "LaunchGemmT":
                labels += [f"Exact<{','.join(a)},{v},{d}>" for v, d in ((0, 0), (1, 0), (1, 1))]
            elif launcher == "LaunchB3":
                labels.append(f"B3<{','.join(a)}>")
            elif launcher == "LaunchB3I":
                labels.append(f"B3I<{','.join(a + ['2'][len(a) - 2:])}>")          # KPS = kKPS = 2
            else:
                labels.append(f"B3J<{','.join(a + ['2', '4', '4'][len(a) - 3:])}>")      # SDIV = 2, MRT = 4, WN = 4
    assert len(set(labels)) == len(labels)
    return labels


def label_of(line: str) -> str:
    m = re.search(r" ((?:Exact|B3|B3I|B3J)<[0-9,]+>) blocks=", line)
    assert m, line
    return m.group(1)


def op_of(line: str) -> str:
    assert line.startswith("gemm_launch: ")
    return line[len("gemm_launch: "):line.index(" rows=")]


# name: net, switches, clip lengths in samples, options; expect: per op (short(): "tdnn2", "tdnnf3.linear", "prefinal", "output", "ivector_lda" for
# the two splice + LDA launches of the iVector branch) what follows the op's name on its `gemm_launch:` line.  Lengths are 400 + 160 (T - 1)
# samples for T frames; the names say T.  What the rows aim at:
#   f33 / f513 / f2049 / f2561 / f2305: one row more than whole tiles -- the last tile of the launch has ONE live row; f576 / f2048: whole tiles;
#   f31 / f127 / f511 / f575 / f1023 / f2047 / f2079 / f2175 / f2431 / f2559 / f2719: one row FEWER -- the last tile (the last small tile of a
#   mixed launch: B3J with nbig = 0, 8 and 16, the 256-row and the narrow shapes, B3I<4,1,2>, B3<4,1,1>; the last 160-row tile at 2559;
#   the exact 64- and 32-row tiles at 127) is one row short of full;
#   f513 (mixed, nbig = 0): a small-tile range of exactly 9 tiles of 64 rows, f512_b3j2 of exactly 8 (every range is padded to 8);
#   f2561: nbig = 16 and nfirst = 8 in front (unclipped: half the 16 slots); f2049_mr4 (the 128-row tile forced): one small tile,
#   nfirst clipped to 0; ragged: utterances of 200, 0, 33, 301 and 1 frames; short_utts: 14 utterances of 40 frames, tiles that cross several;
#   wm2 / mr5 / slots8 / b3i (RS_GEMM_B3J=0 or _SMALL=0) / b3 (RS_GEMM_B3I=0) / excl / exact (RS_GEMM_B3=0) / wide / pad: the switch sets of
#   tests/test_gpu_configs.py at small sizes; fsf3: layers evaluated on every third frame through a strided row list (span unknown: no strip);
#   twide: a row map whose span does not fit the strip (short_utts) and one that does (f600); k32 / k30: KSteps at and under PlanB3J's 32;
#   prune: prune_output_pdfs = 1 -- the library switches pruning off under keep_intermediates (the matrices would lose columns), so the
#   output layer keeps its 362 columns and the row pins that; the option cannot be made effective in a case that reads the launches;
#   resf32 / default f256: folded residual from floats / from the operand image; f256 b3i / b3: the residual pass of GemmKernelB3I / B3.
CASES: Dict[str, dict] = {
    't250_f33': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[5520],
        expect={
            'ivector_lda': 'rows=43 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=1 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=41 n=250 ksteps=10 B3<2,0,1> blocks=8 threads=256 nbig=1 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=39 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=33 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'prefinal': 'rows=33 n=250 ksteps=16 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'output': 'rows=33 n=362 ksteps=16 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
        }),
    't250_f513': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=519 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=513 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=513 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=513 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_f576': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[92400],
        expect={
            'ivector_lda': 'rows=586 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=584 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=582 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=576 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=576 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=576 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_f513_prune': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[82320], opts={'prune_output_pdfs': 1},
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=519 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=513 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=513 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=513 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_ragged': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[32240, 0, 5520, 48400, 400],
        expect={
            'ivector_lda': 'rows=585 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=567 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=559 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=535 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=535 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=535 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_short_utts': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640],
        expect={
            'ivector_lda': 'rows=700 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=672 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=644 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=560 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=560 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=560 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_f1024': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[164080],
        expect={
            'ivector_lda': 'rows=1034 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=24 threads=256 nbig=17 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=1032 n=250 ksteps=10 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=1030 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=24 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=1024 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=1024 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=1024 n=362 ksteps=16 B3J<1,0,0,2,4,4> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f2048': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[327920],
        expect={
            'ivector_lda': 'rows=2058 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2056 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2054 n=250 ksteps=48 B3J<1,0,1,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2048 n=250 ksteps=48 B3J<1,0,1,2,4,4> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2048 n=250 ksteps=16 B3J<1,0,0,2,4,4> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2048 n=362 ksteps=16 B3J<1,0,0,2,4,4> blocks=32 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f2049': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2059 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2057 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2055 n=250 ksteps=48 B3J<1,0,1,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2049 n=250 ksteps=48 B3J<1,0,1,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=48 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f2561': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[410000],
        expect={
            'ivector_lda': 'rows=2571 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=48 threads=256 nbig=41 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2569 n=250 ksteps=10 B3<4,1,1> blocks=32 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2567 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=32 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=2561 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=32 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'prefinal': 'rows=2561 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'output': 'rows=2561 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=64 threads=256 nbig=16 nfirst=8 res=0 img=1',
        }),
    't250_f2049_mr4': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_MR': '4'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2059 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2057 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2055 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2049 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=48 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f31': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[5200],
        expect={
            'ivector_lda': 'rows=41 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=1 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=39 n=250 ksteps=10 B3<2,0,1> blocks=8 threads=256 nbig=1 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=37 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=31 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'prefinal': 'rows=31 n=250 ksteps=16 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'output': 'rows=31 n=362 ksteps=16 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
        }),
    't250_f511_b3j2': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '2'}, clips=[82000],
        expect={
            'ivector_lda': 'rows=521 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=519 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=517 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=511 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=8 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=511 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=8 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=511 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_f575': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[92240],
        expect={
            'ivector_lda': 'rows=585 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=583 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=581 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=575 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=575 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=575 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_f2047': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[327760],
        expect={
            'ivector_lda': 'rows=2057 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2055 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2053 n=250 ksteps=48 B3J<1,0,1,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2047 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=2047 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=2047 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=48 threads=256 nbig=8 nfirst=8 res=0 img=1',
        }),
    't250_f2079_mr4': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_MR': '4'}, clips=[332880],
        expect={
            'ivector_lda': 'rows=2089 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2087 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2085 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2079 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2079 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2079 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=48 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f2719': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[435280],
        expect={
            'ivector_lda': 'rows=2729 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=48 threads=256 nbig=43 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2727 n=250 ksteps=10 B3<4,1,1> blocks=32 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2725 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=32 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=2719 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=32 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'prefinal': 'rows=2719 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'output': 'rows=2719 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=64 threads=256 nbig=16 nfirst=8 res=0 img=1',
        }),
    't250_f2559': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[409680],
        expect={
            'ivector_lda': 'rows=2569 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=48 threads=256 nbig=41 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2567 n=250 ksteps=10 B3<4,1,1> blocks=32 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2565 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=32 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=2559 n=250 ksteps=48 B3J<1,0,1,2,5,4> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2559 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=8 res=0 img=1',
            'output': 'rows=2559 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=48 threads=256 nbig=16 nfirst=8 res=0 img=1',
        }),
    't250_f2047_wm2': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_WM': '2'}, clips=[327760],
        expect={
            'ivector_lda': 'rows=2057 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2055 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2053 n=250 ksteps=48 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2047 n=250 ksteps=48 B3I<4,0,2> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2047 n=250 ksteps=16 B3I<4,0,2> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2047 n=362 ksteps=16 B3J<2,1,0,2,4,4> blocks=32 threads=512 nbig=4 nfirst=0 res=0 img=1',
        }),
    't250_f2175_wm2': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_WM': '2'}, clips=[348240],
        expect={
            'ivector_lda': 'rows=2185 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=35 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2183 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2181 n=250 ksteps=48 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2175 n=250 ksteps=48 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2175 n=250 ksteps=16 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'output': 'rows=2175 n=362 ksteps=16 B3J<2,1,0,2,4,4> blocks=32 threads=512 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f2079_b3i': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '0'}, clips=[332880],
        expect={
            'ivector_lda': 'rows=2089 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2087 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2085 n=250 ksteps=48 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2079 n=250 ksteps=48 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2079 n=250 ksteps=16 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2079 n=362 ksteps=16 B3I<4,1,2> blocks=48 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f575_b3i': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '0'}, clips=[92240],
        expect={
            'ivector_lda': 'rows=585 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=583 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=581 n=250 ksteps=48 B3I<2,0,2> blocks=16 threads=256 nbig=10 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=575 n=250 ksteps=48 B3I<2,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'prefinal': 'rows=575 n=250 ksteps=16 B3I<2,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'output': 'rows=575 n=362 ksteps=16 B3I<4,0,2> blocks=16 threads=256 nbig=5 nfirst=0 res=0 img=1',
        }),
    't250_f2079_b3': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3I': '0'}, clips=[332880],
        expect={
            'ivector_lda': 'rows=2089 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2087 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2085 n=250 ksteps=48 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2079 n=250 ksteps=48 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2079 n=250 ksteps=16 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2079 n=362 ksteps=16 B3<4,1,1> blocks=48 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f1023_b3': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3I': '0'}, clips=[163920],
        expect={
            'ivector_lda': 'rows=1033 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=24 threads=256 nbig=17 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=1031 n=250 ksteps=10 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=1029 n=250 ksteps=48 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=1023 n=250 ksteps=48 B3<2,0,1> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=1023 n=250 ksteps=16 B3<2,0,1> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=1023 n=362 ksteps=16 B3<4,0,1> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f127_exact': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3': '0'}, clips=[20560],
        expect={
            'ivector_lda': 'rows=137 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=135 n=250 ksteps=10 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=133 n=250 ksteps=48 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn3': 'rows=127 n=250 ksteps=48 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=2 nfirst=0 res=0 img=0',
            'prefinal': 'rows=127 n=250 ksteps=16 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=2 nfirst=0 res=0 img=0',
            'output': 'rows=127 n=362 ksteps=16 Exact<2,2,2,1,1> blocks=24 threads=256 nbig=2 nfirst=0 res=0 img=0',
        }),
    't128_f2431_cus4': dict(net='t128', env={'RS_GEMM_CUS': '4'}, clips=[389200],
        expect={
            'ivector_lda': 'rows=2441 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=39 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2439 n=128 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2437 n=128 ksteps=24 B3J<2,1,0,2,4,2> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2431 n=128 ksteps=24 B3J<2,1,0,2,4,2> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2431 n=96 ksteps=8 B3J<2,1,0,2,4,2> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
            'output': 'rows=2431 n=130 ksteps=6 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    'x65_f127': dict(net='x65', env={'RS_GEMM_CUS': '8'}, clips=[20560],
        expect={
            'ivector_lda': 'rows=133 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=129 n=65 ksteps=10 Exact<2,2,2,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=127 n=65 ksteps=15 Exact<2,2,2,1,1> blocks=8 threads=256 nbig=2 nfirst=0 res=0 img=0',
            'prefinal': 'rows=127 n=64 ksteps=5 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=2 nfirst=0 res=0 img=0',
            'output': 'rows=127 n=40 ksteps=4 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=2 nfirst=0 res=0 img=0',
        }),
    'f256_f2079': dict(net='f256', env={'RS_GEMM_CUS': '8'}, clips=[332880],
        expect={
            'ivector_lda': 'rows=2095 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2093 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=2092 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=2091 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf3.linear': 'rows=2088 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf3.affine': 'rows=2085 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf4.linear': 'rows=2082 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf4.affine': 'rows=2079 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2079 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2079 n=128 ksteps=16 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
        }),
    't250_f513_mr5': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_MR': '5'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=519 n=250 ksteps=48 B3J<1,0,1,2,5,4> blocks=8 threads=256 nbig=4 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=513 n=250 ksteps=48 B3J<1,0,1,2,5,4> blocks=8 threads=256 nbig=4 nfirst=0 res=0 img=1',
            'prefinal': 'rows=513 n=250 ksteps=16 B3J<1,0,0,2,5,4> blocks=8 threads=256 nbig=4 nfirst=0 res=0 img=1',
            'output': 'rows=513 n=362 ksteps=16 B3J<1,0,0,2,5,4> blocks=16 threads=256 nbig=4 nfirst=0 res=0 img=1',
        }),
    't250_f512_b3j2': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '2'}, clips=[82160],
        expect={
            'ivector_lda': 'rows=522 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=520 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=518 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=512 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=8 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=512 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=8 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=512 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_f2048_wm2': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_WM': '2'}, clips=[327920],
        expect={
            'ivector_lda': 'rows=2058 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2056 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2054 n=250 ksteps=48 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2048 n=250 ksteps=48 B3J<2,0,0,2,4,4> blocks=8 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2048 n=250 ksteps=16 B3J<2,0,0,2,4,4> blocks=8 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'output': 'rows=2048 n=362 ksteps=16 B3J<2,0,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f2049_wm2': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_WM': '2'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2059 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2057 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2055 n=250 ksteps=48 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2049 n=250 ksteps=48 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=250 ksteps=16 B3J<2,1,0,2,4,4> blocks=16 threads=512 nbig=8 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=362 ksteps=16 B3J<2,1,0,2,4,4> blocks=32 threads=512 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f700_slots8': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_SLOTS': '8'}, clips=[112240],
        expect={
            'ivector_lda': 'rows=710 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=12 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=708 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=12 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=706 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=700 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'prefinal': 'rows=700 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'output': 'rows=700 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=4 nfirst=0 res=0 img=1',
        }),
    't250_f33_b3i': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_SMALL': '0'}, clips=[5520],
        expect={
            'ivector_lda': 'rows=43 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=1 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=41 n=250 ksteps=10 B3<2,0,1> blocks=8 threads=256 nbig=1 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=39 n=250 ksteps=48 B3I<1,0,8> blocks=8 threads=256 nbig=2 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=33 n=250 ksteps=48 B3I<1,0,8> blocks=8 threads=256 nbig=2 nfirst=0 res=0 img=1',
            'prefinal': 'rows=33 n=250 ksteps=16 B3I<1,0,8> blocks=8 threads=256 nbig=2 nfirst=0 res=0 img=1',
            'output': 'rows=33 n=362 ksteps=16 B3I<1,0,8> blocks=16 threads=256 nbig=2 nfirst=0 res=0 img=1',
        }),
    't250_f513_b3i': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '0'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=519 n=250 ksteps=48 B3I<2,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=513 n=250 ksteps=48 B3I<2,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'prefinal': 'rows=513 n=250 ksteps=16 B3I<2,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'output': 'rows=513 n=362 ksteps=16 B3I<4,0,2> blocks=16 threads=256 nbig=5 nfirst=0 res=0 img=1',
        }),
    't250_f1025_b3i': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '0'}, clips=[164240],
        expect={
            'ivector_lda': 'rows=1035 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=24 threads=256 nbig=17 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=1033 n=250 ksteps=10 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=1031 n=250 ksteps=48 B3I<4,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=1025 n=250 ksteps=48 B3I<4,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'prefinal': 'rows=1025 n=250 ksteps=16 B3I<4,0,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'output': 'rows=1025 n=362 ksteps=16 B3I<4,1,2> blocks=32 threads=256 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f2049_b3i': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '0'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2059 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2057 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2055 n=250 ksteps=48 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2049 n=250 ksteps=48 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=250 ksteps=16 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=362 ksteps=16 B3I<4,1,2> blocks=48 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f129_b3': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3I': '0'}, clips=[20880],
        expect={
            'ivector_lda': 'rows=139 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=137 n=250 ksteps=10 B3<2,0,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=135 n=250 ksteps=48 B3<2,0,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=129 n=250 ksteps=48 B3<2,0,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'prefinal': 'rows=129 n=250 ksteps=16 B3<2,0,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'output': 'rows=129 n=362 ksteps=16 B3<2,0,1> blocks=16 threads=256 nbig=3 nfirst=0 res=0 img=1',
        }),
    't250_f1025_b3': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3I': '0'}, clips=[164240],
        expect={
            'ivector_lda': 'rows=1035 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=24 threads=256 nbig=17 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=1033 n=250 ksteps=10 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=1031 n=250 ksteps=48 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=1025 n=250 ksteps=48 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'prefinal': 'rows=1025 n=250 ksteps=16 B3<3,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'output': 'rows=1025 n=362 ksteps=16 B3<4,1,1> blocks=32 threads=256 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f2049_b3': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3I': '0'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2059 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2057 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2055 n=250 ksteps=48 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2049 n=250 ksteps=48 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=250 ksteps=16 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=362 ksteps=16 B3<4,1,1> blocks=48 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't250_f2561_b3_cus4': dict(net='t250', env={'RS_GEMM_CUS': '4', 'RS_GEMM_B3I': '0'}, clips=[410000],
        expect={
            'ivector_lda': 'rows=2571 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=48 threads=256 nbig=41 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2569 n=250 ksteps=10 B3<4,0,1> blocks=24 threads=256 nbig=21 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2567 n=250 ksteps=48 B3<4,0,1> blocks=24 threads=256 nbig=21 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2561 n=250 ksteps=48 B3<4,0,1> blocks=24 threads=256 nbig=21 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2561 n=250 ksteps=16 B3<4,0,1> blocks=24 threads=256 nbig=21 nfirst=0 res=0 img=1',
            'output': 'rows=2561 n=362 ksteps=16 B3<4,1,1> blocks=64 threads=256 nbig=20 nfirst=0 res=0 img=1',
        }),
    't250_f129_excl': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3_EXCLUSIVE': '1'}, clips=[20880],
        expect={
            'ivector_lda': 'rows=139 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=137 n=250 ksteps=10 B3<2,0,2> blocks=8 threads=512 nbig=2 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=135 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=129 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'prefinal': 'rows=129 n=250 ksteps=16 B3J<1,1,0,4,4,4> blocks=8 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'output': 'rows=129 n=362 ksteps=16 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
        }),
    't250_f1025_excl': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3_EXCLUSIVE': '1'}, clips=[164240],
        expect={
            'ivector_lda': 'rows=1035 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=24 threads=256 nbig=17 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=1033 n=250 ksteps=10 B3<3,0,2> blocks=8 threads=512 nbig=6 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=1031 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=24 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=1025 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=24 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=1025 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=1025 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=8 nfirst=0 res=0 img=1',
        }),
    't250_f129_exact': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3': '0'}, clips=[20880],
        expect={
            'ivector_lda': 'rows=139 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=137 n=250 ksteps=10 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=135 n=250 ksteps=48 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn3': 'rows=129 n=250 ksteps=48 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'prefinal': 'rows=129 n=250 ksteps=16 Exact<2,2,2,1,1> blocks=16 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'output': 'rows=129 n=362 ksteps=16 Exact<3,2,2,1,1> blocks=24 threads=256 nbig=2 nfirst=0 res=0 img=0',
        }),
    't250_f700_exact': dict(net='t250', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3': '0'}, clips=[112240],
        expect={
            'ivector_lda': 'rows=710 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=12 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=708 n=250 ksteps=10 Exact<2,2,2,1,1> blocks=32 threads=256 nbig=12 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=706 n=250 ksteps=48 Exact<2,2,2,1,1> blocks=32 threads=256 nbig=12 nfirst=0 res=0 img=0',
            'tdnn3': 'rows=700 n=250 ksteps=48 Exact<2,2,2,1,1> blocks=32 threads=256 nbig=11 nfirst=0 res=0 img=0',
            'prefinal': 'rows=700 n=250 ksteps=16 Exact<2,2,2,1,1> blocks=32 threads=256 nbig=11 nfirst=0 res=0 img=0',
            'output': 'rows=700 n=362 ksteps=16 Exact<3,2,2,1,1> blocks=24 threads=256 nbig=8 nfirst=0 res=0 img=0',
        }),
    't250_f1600_fsf3': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[256240], opts={'frame_subsampling_factor': 3},
        expect={
            'ivector_lda': 'rows=1610 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=32 threads=256 nbig=26 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=1608 n=250 ksteps=10 B3<4,0,1> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=536 n=250 ksteps=48 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=534 n=250 ksteps=48 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=534 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=534 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't250_short_fsf3': dict(net='t250', env={'RS_GEMM_CUS': '8'}, clips=[6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 48240], opts={'frame_subsampling_factor': 3},
        expect={
            'ivector_lda': 'rows=1010 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=980 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=326 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=296 n=250 ksteps=48 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'prefinal': 'rows=296 n=250 ksteps=16 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'output': 'rows=296 n=362 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
        }),
    't256_f513': dict(net='t256', env={'RS_GEMM_CUS': '8'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=256 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=519 n=256 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=513 n=256 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=513 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=513 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't256_f2049': dict(net='t256', env={'RS_GEMM_CUS': '8'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2059 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2057 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2055 n=256 ksteps=48 B3J<1,0,1,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2049 n=256 ksteps=48 B3J<1,0,1,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't128_f257': dict(net='t128', env={'RS_GEMM_CUS': '8'}, clips=[41360],
        expect={
            'ivector_lda': 'rows=267 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=5 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=265 n=128 ksteps=10 B3<2,0,1> blocks=8 threads=256 nbig=5 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=263 n=128 ksteps=24 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=257 n=128 ksteps=24 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'prefinal': 'rows=257 n=96 ksteps=8 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'output': 'rows=257 n=130 ksteps=6 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
        }),
    't128_f513': dict(net='t128', env={'RS_GEMM_CUS': '8'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=128 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=519 n=128 ksteps=24 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=513 n=128 ksteps=24 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'prefinal': 'rows=513 n=96 ksteps=8 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'output': 'rows=513 n=130 ksteps=6 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't128_f2305_cus4': dict(net='t128', env={'RS_GEMM_CUS': '4'}, clips=[369040],
        expect={
            'ivector_lda': 'rows=2315 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=37 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2313 n=128 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2311 n=128 ksteps=24 B3J<2,1,0,2,4,2> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2305 n=128 ksteps=24 B3J<2,1,0,2,4,2> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2305 n=96 ksteps=8 B3J<2,1,0,2,4,2> blocks=16 threads=256 nbig=8 nfirst=0 res=0 img=1',
            'output': 'rows=2305 n=130 ksteps=6 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    't128_f513_wide': dict(net='t128', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J_NARROW': '0'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=128 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=519 n=128 ksteps=24 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=513 n=128 ksteps=24 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=513 n=96 ksteps=8 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=513 n=130 ksteps=6 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
    't128_f513_pad': dict(net='t128', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3_NARROW': '0'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=523 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=521 n=128 ksteps=10 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=6 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=519 n=128 ksteps=24 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=6 nfirst=0 res=0 img=0',
            'tdnn3': 'rows=513 n=128 ksteps=24 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=6 nfirst=0 res=0 img=0',
            'prefinal': 'rows=513 n=96 ksteps=8 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=6 nfirst=0 res=0 img=0',
            'output': 'rows=513 n=130 ksteps=6 Exact<2,2,2,1,1> blocks=32 threads=256 nbig=9 nfirst=0 res=0 img=0',
        }),
    't100_f513': dict(net='t100', env={'RS_GEMM_CUS': '8'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=521 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=519 n=100 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=517 n=100 ksteps=21 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=513 n=100 ksteps=21 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'prefinal': 'rows=513 n=250 ksteps=7 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=513 n=100 ksteps=16 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
        }),
    't100_f2049': dict(net='t100', env={'RS_GEMM_CUS': '8'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2057 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2055 n=100 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2053 n=100 ksteps=21 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn3': 'rows=2049 n=100 ksteps=21 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=250 ksteps=7 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=100 ksteps=16 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
        }),
    'tfar_f600': dict(net='tfar', env={'RS_GEMM_CUS': '8'}, clips=[96240],
        expect={
            'ivector_lda': 'rows=682 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=680 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=600 n=250 ksteps=48 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=600 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=600 n=80 ksteps=16 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=7 nfirst=0 res=0 img=0',
        }),
    'tfar_f2049': dict(net='tfar', env={'RS_GEMM_CUS': '8'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2131 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=34 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2129 n=250 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=2049 n=250 ksteps=48 B3J<1,0,0,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=80 ksteps=16 Exact<3,2,2,1,1> blocks=24 threads=256 nbig=22 nfirst=0 res=0 img=0',
        }),
    'twide_short_utts': dict(net='twide', env={'RS_GEMM_CUS': '8'}, clips=[6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640, 6640],
        expect={
            'ivector_lda': 'rows=1512 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=24 threads=256 nbig=24 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=1484 n=250 ksteps=10 B3<3,0,1> blocks=16 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=644 n=250 ksteps=48 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=560 n=250 ksteps=48 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=560 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=560 n=80 ksteps=16 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=6 nfirst=0 res=0 img=0',
        }),
    'twide_f600': dict(net='twide', env={'RS_GEMM_CUS': '8'}, clips=[96240],
        expect={
            'ivector_lda': 'rows=668 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=666 n=250 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=606 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=600 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=600 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=600 n=80 ksteps=16 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=7 nfirst=0 res=0 img=0',
        }),
    'x65_f129': dict(net='x65', env={'RS_GEMM_CUS': '8'}, clips=[20880],
        expect={
            'ivector_lda': 'rows=135 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=131 n=65 ksteps=10 Exact<2,2,2,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=129 n=65 ksteps=15 Exact<2,2,2,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'prefinal': 'rows=129 n=64 ksteps=5 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'output': 'rows=129 n=40 ksteps=4 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
        }),
    'x65_f700': dict(net='x65', env={'RS_GEMM_CUS': '8'}, clips=[112240, 0, 400],
        expect={
            'ivector_lda': 'rows=719 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=12 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=705 n=65 ksteps=10 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=8 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=701 n=65 ksteps=15 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=8 nfirst=0 res=0 img=0',
            'prefinal': 'rows=701 n=64 ksteps=5 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=0',
            'output': 'rows=701 n=40 ksteps=4 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=11 nfirst=0 res=0 img=0',
        }),
    'x270_f129': dict(net='x270', env={'RS_GEMM_CUS': '8'}, clips=[20880],
        expect={
            'ivector_lda': 'rows=135 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=131 n=270 ksteps=10 Exact<3,2,2,1,1> blocks=24 threads=256 nbig=2 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=129 n=270 ksteps=51 Exact<3,2,2,1,1> blocks=24 threads=256 nbig=2 nfirst=0 res=0 img=0',
            'prefinal': 'rows=129 n=328 ksteps=17 B3J<1,1,0,4,4,4> blocks=16 threads=256 nbig=0 nfirst=0 res=0 img=1',
            'output': 'rows=129 n=80 ksteps=21 Exact<2,2,2,1,1> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=0',
        }),
    'x270_f700': dict(net='x270', env={'RS_GEMM_CUS': '8'}, clips=[112240],
        expect={
            'ivector_lda': 'rows=706 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=12 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=702 n=270 ksteps=10 Exact<3,2,2,1,1> blocks=24 threads=256 nbig=8 nfirst=0 res=0 img=0',
            'tdnn2': 'rows=700 n=270 ksteps=51 Exact<3,2,2,1,1> blocks=24 threads=256 nbig=8 nfirst=0 res=0 img=0',
            'prefinal': 'rows=700 n=328 ksteps=17 B3J<1,1,0,2,4,4> blocks=32 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=700 n=80 ksteps=21 Exact<3,2,2,1,1> blocks=8 threads=256 nbig=8 nfirst=0 res=0 img=0',
        }),
    'f256_f513': dict(net='f256', env={'RS_GEMM_CUS': '8'}, clips=[82320],
        expect={
            'ivector_lda': 'rows=529 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=527 n=256 ksteps=10 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=526 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=525 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnnf3.linear': 'rows=522 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'tdnnf3.affine': 'rows=519 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnnf4.linear': 'rows=516 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
            'tdnnf4.affine': 'rows=513 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=513 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=513 n=128 ksteps=16 B3J<2,0,0,2,4,2> blocks=8 threads=256 nbig=3 nfirst=0 res=0 img=1',
        }),
    'f256_f2049': dict(net='f256', env={'RS_GEMM_CUS': '8'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2065 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2063 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=2062 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=2061 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf3.linear': 'rows=2058 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf3.affine': 'rows=2055 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf4.linear': 'rows=2052 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf4.affine': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=128 ksteps=16 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
        }),
    'f256_f2049_resf32': dict(net='f256', env={'RS_GEMM_CUS': '8', 'RS_RESIDUAL_IMAGE': '0'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2065 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2063 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=2062 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=2061 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf3.linear': 'rows=2058 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf3.affine': 'rows=2055 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf4.linear': 'rows=2052 n=128 ksteps=32 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnnf4.affine': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=128 ksteps=16 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
        }),
    'f256_f2049_b3i': dict(net='f256', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3J': '0'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2065 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2063 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=2062 n=128 ksteps=32 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=2061 n=256 ksteps=16 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=1 img=1',
            'tdnnf3.linear': 'rows=2058 n=128 ksteps=32 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf3.affine': 'rows=2055 n=256 ksteps=16 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=1 img=1',
            'tdnnf4.linear': 'rows=2052 n=128 ksteps=32 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf4.affine': 'rows=2049 n=256 ksteps=16 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=1 img=1',
            'prefinal': 'rows=2049 n=256 ksteps=16 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=128 ksteps=16 B3I<4,1,2> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    'f256_f2049_b3': dict(net='f256', env={'RS_GEMM_CUS': '8', 'RS_GEMM_B3I': '0'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2065 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2063 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=2062 n=128 ksteps=32 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=2061 n=256 ksteps=16 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=1 img=1',
            'tdnnf3.linear': 'rows=2058 n=128 ksteps=32 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf3.affine': 'rows=2055 n=256 ksteps=16 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=1 img=1',
            'tdnnf4.linear': 'rows=2052 n=128 ksteps=32 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf4.affine': 'rows=2049 n=256 ksteps=16 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=1 img=1',
            'prefinal': 'rows=2049 n=256 ksteps=16 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=128 ksteps=16 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
        }),
    'f256_k32_f2049': dict(net='f256_k32', env={'RS_GEMM_CUS': '8'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2057 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2055 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=2052 n=256 ksteps=32 B3J<1,0,0,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=2049 n=256 ksteps=32 B3J<1,0,0,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=128 ksteps=16 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
        }),
    'f256_k30_f2049': dict(net='f256_k30', env={'RS_GEMM_CUS': '8'}, clips=[328080],
        expect={
            'ivector_lda': 'rows=2057 n=12 ksteps=18 Exact<1,4,1,1,1> blocks=40 threads=256 nbig=33 nfirst=0 res=0 img=0',
            'tdnn1': 'rows=2055 n=256 ksteps=10 B3<4,1,1> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'tdnnf2.linear': 'rows=2052 n=240 ksteps=32 B3J<1,0,0,2,5,4> blocks=16 threads=256 nbig=13 nfirst=0 res=0 img=1',
            'tdnnf2.affine': 'rows=2049 n=256 ksteps=30 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'prefinal': 'rows=2049 n=256 ksteps=16 B3J<1,1,0,2,4,4> blocks=24 threads=256 nbig=16 nfirst=0 res=0 img=1',
            'output': 'rows=2049 n=128 ksteps=16 B3J<2,0,0,2,4,2> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
        }),
    't250_noiv_f513': dict(net='t250_noiv', env={'RS_GEMM_CUS': '8'}, clips=[82320, 5520],
        expect={
            'tdnn1': 'rows=562 n=250 ksteps=9 B3<2,0,1> blocks=16 threads=256 nbig=9 nfirst=0 res=0 img=1',
            'tdnn2': 'rows=558 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'tdnn3': 'rows=546 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'prefinal': 'rows=546 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
            'output': 'rows=546 n=250 ksteps=16 B3J<1,1,0,2,4,4> blocks=16 threads=256 nbig=0 nfirst=8 res=0 img=1',
        }),
}

# Incremental streams (8192-byte pieces, a partial result after each): the advances are launches of a few hundred rows.  labels: what
# every image-fed launch of an advance must be.  The baseline of the bit-for-bit comparison is the same stream with RS_GEMM_B3J_SMALL=0
# (GemmKernelB3I<1, false, 8>), as test_small_launches_on_the_all_dma_gemm_are_bitwise_the_image_gemm runs it at full size.
STREAM_CASES: Dict[str, dict] = {
    "t250": dict(net="t250", env={}, samples=48000, labels=("B3J<1,1,0,4,4,4>",)),
    "t250_b3i": dict(net="t250", env={"RS_GEMM_B3J_SMALL": "0"}, samples=48000, labels=("B3I<1,0,8>",)),
    "t128": dict(net="t128", env={}, samples=40000, labels=("B3J<1,1,0,4,4,4>",)),
    "f256": dict(net="f256", env={}, samples=48000, labels=("B3J<1,1,0,4,4,4>",)),
    "f256_resf32": dict(net="f256", env={"RS_RESIDUAL_IMAGE": "0"}, samples=48000, labels=("B3J<1,1,0,4,4,4>",)),
    "t250_noiv": dict(net="t250_noiv", env={}, samples=48000, labels=("B3J<1,1,0,4,4,4>",)),
}


def expected_lines(case: dict) -> List[str]:
    """The `gemm_launch:` lines of a case in the order the call launches them."""
    names = {short(o["name"]): o["name"] for o in net_ops(spec_of(case["net"]))}
    names["ivector_lda"] = LDA_OP
    return [f"gemm_launch: {names[k]} {v}" for k, v in case["expect"].items()]


def is_exact_case(case: dict) -> bool:
    """Every layer of the case runs on the exact-FP32 kernels."""
    return all(v.split(" ")[3].startswith("Exact<") for v in case["expect"].values())
