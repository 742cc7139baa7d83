// The layer GEMM's launch policy (gemm_launch.h), top to bottom: the switches, the rules that say which kernel family can take a
// layer, one cost model per family, the grid.  Measurements behind the constants: DESIGN.md sections 5 and 7, profiles/.
#include "gemm_launch.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "env.h"

namespace rs {
namespace {

using b3::kB3BN;
using b3::kB3KS;

// ------------------------------------------------------------------------------------------ switches
const char *Env(const char *name) { return std::getenv(name); }
bool IsZero(const char *e) { return e && std::atoi(e) == 0; }
int IntOr(const char *e, int unset) { return e ? std::atoi(e) : unset; }

GemmSwitches ReadTuneSwitches() {
  GemmSwitches t;
  t.dma = IntOr(TuneEnv("RS_GEMM_DMA"), t.dma);
  t.narrow_bm = IntOr(TuneEnv("RS_GEMM_NARROW_BM"), t.narrow_bm);
  t.bm = IntOr(TuneEnv("RS_GEMM_BM"), t.bm);
  t.b3_mr = IntOr(TuneEnv("RS_GEMM_B3_MR"), t.b3_mr);
  t.b3_mixed = IntOr(TuneEnv("RS_GEMM_B3_MIXED"), t.b3_mixed);
  t.b3_pad = IntOr(TuneEnv("RS_GEMM_B3_PAD"), t.b3_pad);
  if (const char *e = TuneEnv("RS_GEMM_B3I_EFF64")) t.b3i_eff64 = std::atof(e);
  if (const char *e = TuneEnv("RS_GEMM_B3I_EFF32")) t.b3i_eff32 = std::atof(e);
  t.b3i_kps = IntOr(TuneEnv("RS_GEMM_B3I_KPS"), t.b3i_kps);
  t.b3j_stagger = IntOr(TuneEnv("RS_GEMM_B3J_STAGGER"), t.b3j_stagger);
  return t;
}

bool ImagesEnabled(const GemmSwitches &sw) { return sw.b3i && sw.b3; }

// ------------------------------------------------------------------------------------------ shared arithmetic
int CeilDiv(int a, int b) { return (a + b - 1) / b; }
int Pad8(int tiles) { return (tiles + 7) / 8 * 8; }      // row tiles are dealt to the 8 XCDs round-robin
int KSteps(const GemmDev &d) {
  int n = 0;
  for (int i = 0; i < d.nsegs; i++) n += CeilDiv(d.segs[i].ncols, kB3KS);
  return n;
}
// workgroups the device runs at a time: per_cu on each CU, shared among `share` launches side by side
long Slots(int per_cu, int num_cu, const GemmDev &d) { return std::max((long)per_cu * num_cu / std::max(d.share, 1), 8L); }
long RoundsOf(long row_tiles, int ncol, long slots) { return (row_tiles * ncol + slots - 1) / slots; }
// full-height row tiles of bm rows that fill whole rounds of the slots; the rows behind them run as small tiles
long WholeRoundTiles(int rows, int bm, int ncol, long slots) { return (long)(rows / bm) * ncol / slots * slots / ncol; }

// The grid of a launch whose shape and nbig are set.  Blocks, in the order every kernel decodes from blockIdx: [nfirst small tiles,]
// the nbig full-height tiles, the remaining small tiles; each range padded to a multiple of 8 row tiles, times the column tiles.
// want_first: small tiles asked to go first (sign: GemmLaunch::nfirst), clipped here to a multiple of 8 of those there are.
GemmLaunch WithGrid(GemmLaunch p, const GemmDev &d, int rows, int want_first = 0) {
  const int ncol = CeilDiv(d.n, p.bn());
  const int rest = std::max(rows - p.nbig * p.bm(), 0), nsmall = p.mixed ? CeilDiv(rest, p.small_bm()) : 0;
  const bool alt = want_first < 0;
  int nfirst = p.mixed ? std::min(std::abs(want_first) / 8 * 8, nsmall / 8 * 8) : 0;
  if (alt && p.nbig < nfirst) nfirst = 0;
  p.nfirst = alt ? -nfirst : nfirst;
  p.blocks = (Pad8(p.nbig) + nfirst + Pad8(std::max(nsmall - nfirst, 0))) * ncol;
  p.threads = 64 * p.wm * p.wn;
  return p;
}

// ------------------------------------------------------------------------------------------ which family can take a layer
bool Aligned16(const GemmDev &d) {      // every segment's rows can be read 16 bytes at a time
  for (int i = 0; i < d.nsegs; i++)
    if ((d.segs[i].ld & 3) || (d.segs[i].col0 & 3) || (reinterpret_cast<uintptr_t>(d.segs[i].src) & 15)) return false;
  return true;
}

// GemmKernelB3: FP32 sources, split-fp16 weights
bool B3Usable(const GemmDev &d, const GemmSwitches &sw) {
  if (!sw.b3 || !d.W3 || d.n3 < kB3BN) return false;
  return GemmB3PaddingOk(d.n, d.n3, sw) && Aligned16(d);
}

// GemmKernelB3I / GemmKernelB3J: every source an operand image whose first column sits on a k-step; interleaved k-steps walk ONE image
bool B3IUsable(const GemmDev &d, const GemmSwitches &sw) {
  if (!ImagesEnabled(sw) || !d.W3I || d.n3 < kB3BN) return false;
  if (!GemmB3PaddingOk(d.n, d.n3, sw)) return false;
  for (int i = 0; i < d.nsegs; i++)
    if (!d.segs[i].img.base || d.segs[i].per_utt || (d.segs[i].col0 % kB3KS) != 0) return false;
  if (d.interleave)
    for (int i = 1; i < d.nsegs; i++) if (d.segs[i].img.base != d.segs[0].img.base) return false;
  return true;
}

long JSlots(const GemmDev &d, int wm, int num_cu, const GemmSwitches &sw) {
  if (sw.b3j_slots) return sw.b3j_slots;
  return Slots(wm == 1 ? 2 : 1, num_cu, d);
}

// Of the image-fed launches GemmKernelB3J takes the large ones: the 256-row tile needs whole rounds to pay off; a launch that 32-row
// tiles finish in one round (a stream advance: a few thousand rows) is planned by PlanB3I -- one tile's worth of time on four times
// as many CUs.
bool B3JTakes(const GemmDev &d, int rows, int num_cu, const GemmSwitches &sw) {
  if (sw.b3j == 0) return false;
  const int ncol = CeilDiv(d.n, kB3BN);
  const long min_default = sw.b3j_wm == 2 ? JSlots(d, 2, num_cu, sw) * 256 / ncol : JSlots(d, 1, num_cu, sw) * 32 / ncol + 1;
  const int min_rows = sw.b3j > 1 ? sw.b3j : (int)std::min<long>(min_default, 1 << 30);
  return rows >= min_rows;
}

// The strip form applies to a layer whose three segments are the same 16-column groups of ONE image at three ascending row offsets
// no more than 64 rows apart (a TDNN layer's splice); with a row map (layers evaluated on the rows somebody reads) only when the tile's
// rows, skipped halo rows included, still fit the strip.
bool JStripOk(const GemmDev &d, const GemmSwitches &sw, int tile_rows) {
  if (!sw.b3j_strip) return false;
  if (!d.interleave || d.nsegs != 3) return false;
  const int span = tile_rows == 128 ? d.row_map_span128 : d.row_map_span160;      // physical rows the tile's list rows reach over
  if (d.row_map && (span <= 0 || span + (d.segs[2].row_off - d.segs[0].row_off) > tile_rows + 64)) return false;
  const GemmSegDev &a = d.segs[0];
  if (!a.img.base || a.per_utt) return false;
  for (int i = 1; i < 3; i++) {
    const GemmSegDev &b = d.segs[i];
    if (b.img.base != a.img.base || b.img.part_bytes != a.img.part_bytes || b.img.nks != a.img.nks || b.img.guard != a.img.guard || b.per_utt ||
        b.col0 != a.col0 || b.ncols != a.ncols || b.row_off <= d.segs[i - 1].row_off)
      return false;
  }
  return a.col0 % kB3KS == 0 && d.segs[2].row_off - a.row_off <= 64;
}

// ------------------------------------------------------------------------------------------ exact FP32
// Tile height: the one whose busiest CU does the least work; at equal work the shorter tile wins (more workgroups per CU hide the
// staging latency better: measured 808 vs 848 us on the output layer for 64- vs 128-row tiles).
GemmLaunch PlanExact(const GemmDev &d, int rows, int num_cu, const GemmSwitches &sw) {
  GemmLaunch p;
  p.family = GemmLaunch::kExact;
  p.vec = Aligned16(d);
  p.dma = p.vec && sw.dma;
  auto cost = [&](int bm, int bn) {
    const long tiles = (long)CeilDiv(rows, bm) * CeilDiv(d.n, bn);
    const double pref = bm == 64 ? 0.97 : (bm == 96 ? 0.985 : 1.0);
    return (double)(((tiles + num_cu - 1) / num_cu) * bm * bn) * pref;
  };
  if (d.n <= 64) {          // four waves stacked on one 64-column tile
    p.wm = 4; p.wn = 1;
    p.mr = (sw.narrow_bm ? sw.narrow_bm == 64 : cost(64, 64) < cost(128, 64)) ? 1 : 2;
  } else {                  // two by two waves, 128 columns
    p.wm = 2; p.wn = 2;
    double c128 = cost(128, 128), c96 = cost(96, 128), c64 = cost(64, 128);
    if (sw.bm == 128) c128 = 0; else if (sw.bm == 96) c96 = 0; else if (sw.bm == 64) c64 = 0;
    p.mr = (c128 <= c96 && c128 <= c64) ? 4 : (c96 <= c64 ? 3 : 2);
  }
  p.nbig = CeilDiv(rows, p.bm());
  return WithGrid(p, d, rows);
}

// ------------------------------------------------------------------------------------------ GemmKernelB3
GemmLaunch PlanB3(const GemmDev &d, int rows, int num_cu, const GemmSwitches &sw) {
  GemmLaunch p;
  p.family = GemmLaunch::kB3;
  p.residual_pass = d.res != nullptr;      // (this kernel's epilogue does not add a folded residual)
  p.writes_image = true;
  const int ncol = CeilDiv(d.n, kB3BN);
  if (d.exclusive) {
    // one 512-thread workgroup per CU; tile height 128 or 192 rows, whichever leaves the fuller last round.
    // (Counts CUs: d.share is ignored here.)
    auto rounds1 = [&](int bm) { return (double)RoundsOf(CeilDiv(rows, bm), ncol, num_cu) * bm; };
    p.wm = 2;
    p.mr = rounds1(192) * 0.97 < rounds1(128) ? 3 : 2;
    p.nbig = CeilDiv(rows, p.bm());
    return WithGrid(p, d, rows);
  }
  const long slots = Slots(2, num_cu, d);      // two workgroups per CU
  // Tile height: rounds of `slots` tiles, each as long as the tile is tall, weighted by the measured per-row efficiency
  // of the height (taller tiles stream the weights for more rows: 0.78 at 128 rows).
  auto rounds = [&](long row_tiles) { return (double)RoundsOf(row_tiles, ncol, slots); };
  auto cost = [&](int bm, double eff) { return rounds(CeilDiv(rows, bm)) * bm * eff; };
  int mr = 2, nbig = CeilDiv(rows, 64);
  double best = cost(64, 1.0);
  if (cost(96, 0.97) < best) { best = cost(96, 0.97); mr = 3; nbig = CeilDiv(rows, 96); }
  if (cost(128, 0.78) < best) { best = cost(128, 0.78); mr = 4; nbig = CeilDiv(rows, 128); }
  if (sw.b3_mixed) {
    // whole rounds of 128-row tiles, the remaining rows as 64-row tiles of the same launch
    const long full = WholeRoundTiles(rows, 128, ncol, slots), rest = rows - full * 128;
    const double c = rounds(full) * 128 * 0.78 + rounds((rest + 63) / 64) * 64 * 1.0;
    if (full > 0 && c < best) { best = c; mr = 4; nbig = (int)full; }
  }
  if (sw.b3_mr >= 2 && sw.b3_mr <= 4) { mr = sw.b3_mr; nbig = CeilDiv(rows, 32 * mr); }
  p.mr = mr;
  p.nbig = nbig;
  p.mixed = mr == 4 && (long)nbig * 128 < rows;
  return WithGrid(p, d, rows);
}

// ------------------------------------------------------------------------------------------ GemmKernelB3I, and 32-row tiles on GemmKernelB3J
GemmLaunch PlanB3I(const GemmDev &d, int rows, int num_cu, const GemmSwitches &sw) {
  GemmLaunch p;
  p.family = GemmLaunch::kB3I;
  p.writes_image = true;
  const int ncol = CeilDiv(d.n, kB3BN);
  const long slots = Slots(2, num_cu, d);      // two workgroups per CU
  // Tile height: rounds of `slots` tiles, each as long as the tile is tall, weighted by the per-row cost of the height
  // (a 64-row tile streams the weights for half as many rows as a 128-row one)
  auto rounds = [&](long row_tiles) { return (double)RoundsOf(row_tiles, ncol, slots); };
  // whole rounds of 128-row tiles, the remaining rows as 64-row tiles of the same launch
  const long full = WholeRoundTiles(rows, 128, ncol, slots), rest = rows - full * 128;
  const double c_mixed = rounds(full) * 128 + rounds((rest + 63) / 64) * 64 * sw.b3i_eff64;
  const double c_128 = rounds(CeilDiv(rows, 128)) * 128, c_64 = rounds(CeilDiv(rows, 64)) * 64 * sw.b3i_eff64;
  // a launch of less than one round (a stream advance: a few thousand rows) is as long as ONE tile is: the 32-row tile spreads it
  // over four times as many CUs as the 128-row one, each streaming the same weights for a quarter of the rows
  const double c_32 = rounds(CeilDiv(rows, 32)) * 32 * sw.b3i_eff32;
  int mr = 4;
  bool mixed = false;
  if (c_32 < c_64 && c_32 < c_128 && c_32 <= c_mixed) mr = 1;
  else if (c_64 < c_128 && c_64 <= c_mixed) mr = 2;
  else if (full > 0 && c_mixed < c_128) mixed = true;
  if (sw.b3_mr == 1 || sw.b3_mr == 2 || sw.b3_mr == 4) { mr = sw.b3_mr; mixed = false; }
  // 32-row tiles run on GemmKernelB3J where it is on (its four-wave shape): GemmKernelB3I's ordinary weight loads are waited for with
  // vmcnt(0) in every k-step, 0.59 us per k-step for a workgroup alone on its CU; there nothing in the loop is a load the compiler
  // sees.  It adds a folded residual itself.  (This cost model chose the 32-row tiles with its own slot count: RS_GEMM_B3J_SLOTS
  // is ignored here.)
  if (mr == 1 && sw.b3j_small && sw.b3j != 0 && sw.b3j_wm == 1) {
    p.family = GemmLaunch::kB3J;
    p.mr = 4; p.mixed = true; p.sdiv = 4;      // no full-height tile: every tile a quarter of 128 rows
    p.nbig = 0;
    return WithGrid(p, d, rows);
  }
  p.residual_pass = d.res != nullptr;      // (this kernel's epilogue does not add a folded residual)
  p.mr = mr;
  p.mixed = mixed;
  p.kps = mr != 1 ? 2 : (sw.b3i_kps == 8 || sw.b3i_kps == 4) ? sw.b3i_kps : 2;      // (the 32-row tile: eight k-steps per LDS stage)
  p.nbig = mixed ? (int)full : CeilDiv(rows, 32 * mr);
  return WithGrid(p, d, rows);
}

// ------------------------------------------------------------------------------------------ GemmKernelB3J
GemmLaunch PlanB3J(const GemmDev &d, int rows, int num_cu, const GemmSwitches &sw) {
  GemmLaunch p;
  p.family = GemmLaunch::kB3J;
  p.writes_image = true;
  p.mr = 4;
  const int wm = sw.b3j_wm;
  const int ncol = CeilDiv(d.n, kB3BN);
  const long slots = JSlots(d, wm, num_cu, sw);
  // Layers of at most 128 columns: the 256 x 128 tile (two wave rows x two wave columns); half of the 256-column shapes' weight
  // stream and MFMAs would be padding for such a layer.  One column tile.
  if (wm == 1 && d.n <= 128 && sw.b3j_narrow) {
    p.wm = 2; p.wn = 2;
    const long full = WholeRoundTiles(rows, 256, 1, slots);
    p.mixed = !(full * 256 >= rows || CeilDiv(rows, 256) <= slots);
    p.nbig = p.mixed ? (int)full : CeilDiv(rows, 256);
    return WithGrid(p, d, rows);
  }
  // The 160-row tile (five row blocks per wave) where it turns a launch of two rounds of tiles into ONE: a tile's k loop is as long as
  // staging its weights takes, whatever its height, so a long-K launch costs about one loop time per round -- the half-height tiles of
  // the last, partly filled round included.  Measured (profiles/r06/notes_experiments.txt): hidden layers (K = 750) 101 -> 90 us; no gain
  // where K is short (the pre-final and output layers, K = 250: the tile's time is its epilogue, which grows with its rows) or where
  // the taller tiles still need several rounds.
  if (wm == 1) {
    const long rounds4 = RoundsOf(CeilDiv(rows, 128), ncol, slots), rounds5 = RoundsOf(CeilDiv(rows, 160), ncol, slots);
    if (sw.b3j_mr == 5 || (sw.b3j_mr != 4 && rounds5 == 1 && rounds4 > 1 && KSteps(d) >= 32)) {
      p.mr = 5;
      p.strip = JStripOk(d, sw, 160);
      p.nbig = CeilDiv(rows, 160);
      return WithGrid(p, d, rows);
    }
  }
  // whole rounds of full-height tiles; the remaining rows as half-height tiles of the same launch, some of them in front: with all
  // tiles of a round the same height every workgroup reaches its epilogue at the same moment (nnet_gemm_b3j.hip: block order)
  p.wm = wm;
  p.strip = wm == 1 && JStripOk(d, sw, 128);
  const int bm = 128 * wm;
  const long full = WholeRoundTiles(rows, bm, ncol, slots);
  p.mixed = full * bm < rows;
  p.nbig = p.mixed ? (int)full : CeilDiv(rows, bm);
  int nfirst = sw.b3j_stagger ? (int)(slots / 2) : 0;
  if (sw.b3j_stagger == 2 && p.nbig >= nfirst) nfirst = -nfirst;
  return WithGrid(p, d, rows, nfirst);
}

}  // namespace

GemmSwitches ReadGemmSwitches() {
  static const GemmSwitches tuned = ReadTuneSwitches();      // once per process
  GemmSwitches s = tuned;
  s.b3 = !IsZero(Env("RS_GEMM_B3"));
  s.b3i = !IsZero(Env("RS_GEMM_B3I"));
  s.b3j = IntOr(Env("RS_GEMM_B3J"), 1);
  s.b3j_wm = IntOr(Env("RS_GEMM_B3J_WM"), 1) == 2 ? 2 : 1;
  if (const char *e = Env("RS_GEMM_B3J_SLOTS")) s.b3j_slots = std::max(std::atol(e), 1L);
  s.b3j_mr = IntOr(Env("RS_GEMM_B3J_MR"), 0);
  s.b3j_narrow = !IsZero(Env("RS_GEMM_B3J_NARROW"));
  s.b3j_small = !IsZero(Env("RS_GEMM_B3J_SMALL"));
  s.b3_narrow = !IsZero(Env("RS_GEMM_B3_NARROW"));
  s.cus = std::max(IntOr(Env("RS_GEMM_CUS"), 0), 0);
  s.b3j_strip = !IsZero(TuneEnv("RS_GEMM_B3J_STRIP"));
  return s;
}

bool GemmImagesEnabled() { return !IsZero(Env("RS_GEMM_B3I")) && !IsZero(Env("RS_GEMM_B3")); }

// Up to 45 % of the 256-column tiles may be padding: per padded column the split-fp16 kernels are about three times as fast as
// the exact-FP32 kernel with its 128-column tiles (hidden layer 105 us for 33 GFLOP against 163 us for the 15 GFLOP of the pruned
// output layer, profiles/r04), so e.g. the headline's 362 output columns (29 % padding in two tiles) belong here: 163 -> 85 us.
bool GemmB3PaddingOk(int n, int n3, const GemmSwitches &sw) {
  // One tile wide, at least 96 columns (round 6: a factorised TDNN's 128-wide bottlenecks, K = 2048): the exact-FP32 kernel ran such a
  // layer at 109 TFLOP/s, 0.7 of ITS peak (403 us for 84 k rows), the split kernels take 62.5 % padding and are still 2.4 times as fast
  // (profiles/r06/tdnnf_notes.txt); RS_GEMM_B3_NARROW=0 keeps the 45 % rule alone.
  if (n3 == kB3BN && n >= 96 && sw.b3_narrow) return true;
  return (long)(n3 - n) * 100 <= (long)n3 * sw.b3_pad;
}

bool GemmWritesImage(const GemmDev &d, const GemmSwitches &sw) { return B3IUsable(d, sw) || B3Usable(d, sw); }

GemmLaunch PlanGemmLaunch(const GemmDev &d, int rows, int num_cu, const GemmSwitches &sw) {
  if (B3IUsable(d, sw)) return B3JTakes(d, rows, num_cu, sw) ? PlanB3J(d, rows, num_cu, sw) : PlanB3I(d, rows, num_cu, sw);
  if (B3Usable(d, sw)) return PlanB3(d, rows, num_cu, sw);
  return PlanExact(d, rows, num_cu, sw);
}

const char *DescribeGemmLaunch(const GemmLaunch &p, char *buf, size_t size) {
  int at = 0;
  switch (p.family) {
    case GemmLaunch::kExact: at = std::snprintf(buf, size, "Exact<%d,%d,%d,%d,%d>", p.mr, p.wm, p.wn, (int)p.vec, (int)p.dma); break;
    case GemmLaunch::kB3: at = std::snprintf(buf, size, "B3<%d,%d,%d>", p.mr, (int)p.mixed, p.wm); break;
    case GemmLaunch::kB3I: at = std::snprintf(buf, size, "B3I<%d,%d,%d>", p.mr, (int)p.mixed, p.kps); break;
    case GemmLaunch::kB3J: at = std::snprintf(buf, size, "B3J<%d,%d,%d,%d,%d,%d>", p.wm, (int)p.mixed, (int)p.strip, p.sdiv, p.mr, p.wn); break;
  }
  if (at >= 0 && (size_t)at < size)
    std::snprintf(buf + at, size - at, " blocks=%d threads=%d nbig=%d nfirst=%d res=%d", p.blocks, p.threads, p.nbig, p.nfirst, (int)p.residual_pass);
  return buf;
}

const char *DescribeGemmLaunchLine(const char *name, const GemmDev &d, int rows, const GemmLaunch &p, char *buf, size_t size) {
  char launch[200];
  std::snprintf(buf, size, "%s rows=%d n=%d ksteps=%d %s img=%d", name, rows, d.n, KSteps(d), DescribeGemmLaunch(p, launch, sizeof(launch)), (int)p.writes_image);
  return buf;
}

}  // namespace rs
