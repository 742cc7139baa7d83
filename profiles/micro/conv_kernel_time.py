"""The convolution kernel alone on recipe-size layers (1->64 and 64->64 filters on 40 heights, 64->128 to 20 heights, 128->256 to 10;
3x3 offsets; 256 x 300 rows): builds profiles/micro/conv_kernel_time from conv_kernel_time.hip against the built library, if it is
not there (or when asked to: --build-only), and runs it: per layer the load-time plan, the median and minimum time of the launches after
the warm-up (HIP events, one process) and the fraction of the FP32 matrix-core peak.  Needs the GPU (the build does not).
  usage: python profiles/micro/conv_kernel_time.py [repeats, default 20] [warmup, default 3]     (--build-only: just the build)"""
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
LIB = ROOT / "rhasspy_speech_amd" / "librhasspy_speech_hip.so"
EXE, SRC = HERE / "conv_kernel_time", HERE / "conv_kernel_time.hip"

if not LIB.exists():
    raise SystemExit(f"{LIB} is missing: build the library first")
if not EXE.exists() or "--build-only" in sys.argv[1:]:
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", str(SRC), "-o", str(EXE), f"-L{LIB.parent}", "-l:" + LIB.name,
                    "-Wl,-rpath,$ORIGIN/../../rhasspy_speech_amd"], check=True)
args = [a for a in sys.argv[1:] if a != "--build-only"]
if "--build-only" not in sys.argv[1:]:
    sys.exit(subprocess.run([str(EXE), *args]).returncode)
