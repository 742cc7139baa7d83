// Host-only launch policy of the layer GEMM: which of the four kernels runs a GemmDev, in which template shape, with how many
// full-height and small tiles, in which block order and on how large a grid.  Plain arithmetic on the descriptor, the row count,
// the device's CU count and the RS_GEMM_* switches: nothing here includes a HIP header, launches or allocates, so every decision
// can be checked on a machine without a GPU (tests/host/gemm_launch_check.cc, tests/test_gemm_launch_cpu.py).  The .hip files
// keep the kernels and one function each that maps a GemmLaunch to the matching instantiation (nnet_common.h).
#pragma once
#include <cstddef>

#include "gemm_dev.h"

namespace rs {

// How one launch runs.  The shape fields mirror the kernels' template parameters; a field a family does not have keeps the value
// that makes bm() / bn() below come out right.
struct GemmLaunch {
  enum Family {
    kExact,      // nnet_kernels.hip: GemmKernelDma<MT, WM, WN> (dma), GemmKernel<MT, WM, WN, VEC> (else)
    kB3,         // nnet_gemm_b3.hip: GemmKernelB3<MR, MIXED, WM>, FP32 sources split in the k loop
    kB3I,        // nnet_gemm_b3i.hip: GemmKernelB3I<MR, MIXED, KPS>, sources stored as operand images
    kB3J,        // nnet_gemm_b3j.hip: GemmKernelB3J<WM, MIXED, STRIP, SDIV, MRT, WN>, both operands by LDS-DMA
  } family = kExact;
  int mr = 1;              // row blocks per wave row: MT (16 rows each) of the exact kernels, MR / MRT (32 rows each) of the others
  int wm = 1, wn = 4;      // wave rows; 64-column wave columns (the exact kernels and GemmKernelB3J's narrow shape: else always 4)
  bool vec = false, dma = false;      // exact: 16-byte source loads / direct-to-LDS staging
  bool mixed = false;      // the rows behind the nbig full-height tiles run as small tiles of the same launch
  bool strip = false;      // B3J: one activation strip per 16-column group instead of one fragment set per row offset
  int kps = 0;             // B3I: k-steps per LDS stage
  int sdiv = 2;            // B3J: a small tile is 1 / sdiv of the full height
  int nbig = 0;            // full-height row tiles (the exact kernels: all row tiles)
  int nfirst = 0;          // B3J, mixed: small tiles in front of the full-height ones (a multiple of 8, clipped to what there is);
                           // negative: the first 2 |nfirst| tiles alternate, eight small, eight full-height, ...
  int blocks = 0, threads = 256;
  bool residual_pass = false;      // B3 / B3I: the kernel runs on GemmWithoutResidual(d), LaunchResidualAdd adds d.res behind it
  bool writes_image = false;       // the launch leaves d.out_img written (else the caller converts: LaunchToImage)

  int bm() const { return (family == kExact ? 16 : 32) * mr * wm; }      // rows of a full-height tile
  int small_bm() const { return !mixed ? 0 : family == kB3J ? 32 * wm * (mr / sdiv) : bm() / 2; }
  int bn() const { return 64 * wn; }
};

// The RS_GEMM_* switches a plan depends on (env.h).
struct GemmSwitches {
  // product and test switches: std::getenv on every ReadGemmSwitches() -- tests flip them inside one process
  bool b3 = true;          // RS_GEMM_B3=0: exact-FP32 kernels only
  bool b3i = true;         // RS_GEMM_B3I=0: no operand images
  int b3j = 1;             // RS_GEMM_B3J: 0 = never GemmKernelB3J, > 1 = the smallest launch (rows) it takes
  int b3j_wm = 1;          // RS_GEMM_B3J_WM=2: the 256 x 256 tile
  long b3j_slots = 0;      // RS_GEMM_B3J_SLOTS: pretend the device runs this many workgroups at a time (0: ask the device)
  int b3j_mr = 0;          // RS_GEMM_B3J_MR=4|5: force the 128- / 160-row tile
  bool b3j_narrow = true;  // RS_GEMM_B3J_NARROW=0: layers of at most 128 columns stay on the 256-column shapes
  bool b3j_small = true;   // RS_GEMM_B3J_SMALL=0: launches of 32-row tiles stay on GemmKernelB3I
  bool b3_narrow = true;   // RS_GEMM_B3_NARROW=0: one-tile layers of 96 columns and more obey the padding rule too
  int cus = 0;             // RS_GEMM_CUS: plan as if the device had this many compute units (0: ask the device); grid shapes only
  // measurement switches (TuneEnv: unset unless the build has -DRS_TUNING).  b3j_strip is read on every ReadGemmSwitches(), the
  // others once per process
  bool b3j_strip = true;   // RS_GEMM_B3J_STRIP=0
  int dma = 1;             // RS_GEMM_DMA
  int narrow_bm = 0;       // RS_GEMM_NARROW_BM
  int bm = 0;              // RS_GEMM_BM
  int b3_mr = 0;           // RS_GEMM_B3_MR (GemmKernelB3: 2..4, GemmKernelB3I: 1, 2, 4)
  int b3_mixed = 1;        // RS_GEMM_B3_MIXED
  int b3_pad = 45;         // RS_GEMM_B3_PAD (percent)
  double b3i_eff64 = 1.3;  // RS_GEMM_B3I_EFF64
  double b3i_eff32 = 1.7;  // RS_GEMM_B3I_EFF32
  int b3i_kps = 8;         // RS_GEMM_B3I_KPS
  int b3j_stagger = 1;     // RS_GEMM_B3J_STAGGER
};
GemmSwitches ReadGemmSwitches();

// rows > 0.  num_cu: the device's compute units.  Does not allocate; every GemmDev is valid input.
GemmLaunch PlanGemmLaunch(const GemmDev &d, int rows, int num_cu, const GemmSwitches &sw);

// "B3J<1,1,1,2,4,4> blocks=776 threads=256 nbig=512 nfirst=256 res=0": the kernel's template arguments in their order, then the grid
// (error messages, the CPU check's fixture).  Returns buf.
const char *DescribeGemmLaunch(const GemmLaunch &p, char *buf, size_t size);

// The compute units LaunchGemm plans with: RS_GEMM_CUS where it is set, else the device's.
inline int GemmPlanCus(const GemmSwitches &sw, int device_cus) { return sw.cus > 0 ? sw.cus : device_cus; }

// "<name> rows=81920 n=250 ksteps=48 B3J<1,1,1,2,4,4> blocks=776 ... res=0 img=1": what rs_model_describe prints behind "gemm_launch: "
// for a launch it recorded, and what tests/host/gemm_launch_check.cc prints for a descriptor file.  ksteps: the 16-wide k-steps of the
// split-fp16 kernels' k loop, every segment rounded up on its own; the launch is DescribeGemmLaunch's text; img: p.writes_image.  Returns buf.
const char *DescribeGemmLaunchLine(const char *name, const GemmDev &d, int rows, const GemmLaunch &p, char *buf, size_t size);

// The split-fp16 kernels work on 256-column tiles: a layer takes them only while the padding stays below a share of the
// padded width (45 %; above it the exact-FP32 kernel with its 128-column tiles wins), or is one tile of at least 96 columns.
bool GemmB3PaddingOk(int n, int n3, const GemmSwitches &sw);
inline bool GemmB3PaddingOk(int n, int n3) { return GemmB3PaddingOk(n, n3, ReadGemmSwitches()); }
// whatever the row count, the launch PlanGemmLaunch plans for d leaves d.out_img written (GemmLaunch::writes_image)
bool GemmWritesImage(const GemmDev &d, const GemmSwitches &sw);
// RS_GEMM_B3I / RS_GEMM_B3, read now: layers may be fed by operand images at all
bool GemmImagesEnabled();

}  // namespace rs
