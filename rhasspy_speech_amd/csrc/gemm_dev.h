// The descriptor of one layer GEMM (kernels.h: LaunchGemm) as plain structs: nothing here includes a HIP header, so the host-only
// launch policy (gemm_launch.h) and its CPU check (tests/host/gemm_launch_check.cc) see the same type the kernels take by value.
#pragma once
#include <cstddef>

namespace rs {

// ---------------------------------------------------------------- generic segmented GEMM (FP32 MFMA)
constexpr int kGemmBM = 128, kGemmBN = 128, kGemmBK = 32;
namespace b3 {
constexpr int kB3BN = 256, kB3KS = 16;      // the split-fp16 kernels' column tile and k-step (nnet_b3_common.h)
}
// A frame buffer stored a second time in the operand order of the fp16 matrix cores, already split into the two fp16
// parts of nnet_gemm_b3.hip: part p at base + p * part_bytes, inside a part [row block of 32][16-wide k-step][k-group 2]
// [row 32][8 fp16] -- one 1 KiB block is one A fragment of v_mfma_f32_32x32x16_f16 (lane l: row l & 31, k-group l >> 5).
// Image row = buffer row + guard (a multiple of 32); columns beyond the buffer's width up to 16 * nks are zero.
struct ActImage {
  unsigned char *base;
  size_t part_bytes;
  int nks;
  int guard;
};
struct GemmSegDev {
  ActImage img;       // the source buffer's operand image (base null: none)
  const float *src;   // source buffer base (row 0 of the frame buffer), or iVector matrix if per_utt
  int ld;             // leading dimension of the source
  int col0;           // first source column
  int ncols;          // valid K extent
  int row_off;        // constant row offset (time offset)
  int k0;             // first (padded) K index of this segment inside W
  int per_utt;        // 1: row index = row_ivec[row] (iVector input: one row per utterance, or per nnet chunk when streaming)
};
constexpr int kMaxSegs = 16;
struct EltStageDev {
  int kind;                 // 0 relu, 1 scale+offset, 4 scalar scale
  const float *scale, *offset;
  float alpha;
};
constexpr int kMaxStages = 6;
struct GemmDev {
  int nsegs;
  GemmSegDev segs[kMaxSegs];
  const float *W;     // n_pad x k_pad, row-major, zero padded (k_pad = sum of segment widths rounded to kGemmBK)
  int k_pad, n, n_pad;
  const void *W3;     // the same weights, every output column scaled by a power of two (w3_inv_scale) and split into two fp16 parts in MFMA fragment order (nnet_gemm_b3.hip), or null
  const void *W3I;    // the same for GemmKernelB3I: segments padded to the 16-wide k-step instead of to kGemmBK, or null
  const float *w3_inv_scale;   // n3 floats: what the accumulators of column c are multiplied by (the inverse of W3's column scale)
  int *ovf;           // two words.  [0]: set to 1 by a kernel that met an activation the fp16 split cannot carry (|x| >= 65520 or not a number);
                      // [1]: ... that split an operand row whose largest element is below 2^-3 (the split would carry it to 2^-25
                      // absolute only, nnet_b3_common.h).  Either way the host repeats the call on the exact-FP32 kernels
  int n3;             // columns of W3 (n rounded up to 256)
  int interleave;     // 1: W3's k-steps alternate between the segments (all segments shifted views of one buffer)
  int exclusive;      // 1: GemmKernelB3 keeps every other workgroup off its CU (several decode pipelines in flight)
  int share;          // launches of this kind that run side by side on the device (sub-batch groups): tile planning hint
  const float *bias;  // n (may be null)
  int nstages;
  EltStageDev stages[kMaxStages];
  float *out;
  int ldo;
  // null, or the rows of a buffer as wide as the result: out = stages(...) + res_scale * res[same row] (a residual sum folded into the
  // layer, LayerOp::res_buf), the product and the sum rounded like the elementwise kernel's (__fmul_rn, __fadd_rn)
  const float *res;
  int res_ld;
  float res_scale;
  // base non-null (split-fp16 kernels fed by operand images): the residual's rows are taken from ITS operand image instead -- the sum of
  // the two fp16 parts, i.e. the value the next layer's GEMM multiplies, within 2^-22 of the FP32 number (nnet_b3_common.h) -- so a
  // chain of residual layers needs no FP32 copy of its activations at all (half the epilogue's traffic, no pass through LDS)
  ActImage res_img;
  ActImage out_img;    // base non-null: the result is (also) written as an operand image for the layers that consume it
  int write_f32;       // 0: nobody reads `out` as floats (every consumer takes the image): skip that store
  const int *row_map;  // null, or rows entries: GEMM row i reads / writes physical row row_map[i] (e.g. only the real frames)
  int row_map_span128; // with a row map: an upper bound of row_map[i + 127] - row_map[i] + 1 over the list when the list is ascending (128 rows of
                       // a tile reach over that many physical rows: GemmKernelB3J stages them as one strip), 0 = not known
  int row_map_span160; // the same for 160 consecutive rows of the list (the 160-row tile)
};

}  // namespace rs
