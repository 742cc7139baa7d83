// Stand-alone check of csrc/gemm_launch.{h,cc} (tests/test_gemm_launch_cpu.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers, and runs it as a child process).  Fabricates the GemmDev of a set of layers -- pointers are made-up
// addresses, never dereferenced -- and walks a sweep of row counts, `share`, `exclusive` and RS_GEMM_* settings.  The switches are
// set in the environment, so ReadGemmSwitches is part of what is checked; the device has 256 CUs.  One line per case:
//     <layer> <rows> s<share> x<exclusive> <switches without their RS_GEMM_ prefix, or -> | <DescribeGemmLaunch> img=<GemmWritesImage>
// compared by the test with tests/host/gemm_launch_expected.txt.
// With an argument (tests/test_gemm_shapes_cpu.py): the name of a text file of descriptors, one per line, as tests/gemm_shape_cases.py
// writes them (ReadDescriptor below).  For each the program plans the launch with the line's CU count and switches, runs the same
// coverage check and prints "gemm_launch: " and DescribeGemmLaunchLine -- the line rs_model_describe prints for a launch it recorded.
// For every case the program also restates how the kernels decode blockIdx (XCD-interleaved row tiles; the first-small, full and
// remaining-small ranges of a mixed launch; the alternating order of a negative nfirst) and aborts unless every (row, column tile)
// of [0, rows) x [0, ncol) belongs to exactly one block of the planned grid.
//
// The expected file is a recording of the launch code as it was BEFORE the policy moved into gemm_launch.cc: that tree's four
// kernel files, with every hipLaunchKernelGGL of a layer GEMM replaced by a snprintf of the template arguments and the grid into
// g_rec (and the residual pass by g_res++), linked with this file compiled with -DGEMM_LAUNCH_RECORD.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#ifdef GEMM_LAUNCH_RECORD
#include "kernels.h"
char g_rec[256];
int g_res;
#else
#include "../../rhasspy_speech_amd/csrc/gemm_launch.h"
#endif

using namespace rs;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "gemm_launch_check: %s failed: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::abort(); } } while (0)

// ---------------------------------------------------------------------------------------------- layers
template <typename T> static T *Fake(uintptr_t a) { return reinterpret_cast<T *>(a); }
static const ActImage kImgA{Fake<unsigned char>(0x10000000), 1 << 24, 16, 64}, kImgB{Fake<unsigned char>(0x30000000), 1 << 24, 16, 64};

static GemmDev Base(int n, bool w3, bool w3i) {
  GemmDev d;
  std::memset(&d, 0, sizeof(d));
  d.n = n;
  d.n_pad = (n + 127) / 128 * 128;
  d.n3 = (n + 255) / 256 * 256;
  d.W = Fake<const float>(0x50000000);
  if (w3) d.W3 = Fake<const void>(0x51000000);
  if (w3i) d.W3I = Fake<const void>(0x52000000);
  d.share = 1;
  d.write_f32 = 1;
  d.res_scale = 1.0f;
  d.out = Fake<float>(0x60000000);
  d.ldo = d.n_pad;
  return d;
}
static void Seg(GemmDev *d, const ActImage *img, int ld, int col0, int ncols, int row_off, int per_utt = 0, uintptr_t src = 0x20000000) {
  GemmSegDev &s = d->segs[d->nsegs++];
  if (img) s.img = *img;
  s.src = Fake<const float>(src);
  s.ld = ld; s.col0 = col0; s.ncols = ncols; s.row_off = row_off; s.per_utt = per_utt;
  s.k0 = d->k_pad;
  d->k_pad += (ncols + 31) / 32 * 32;
}
// the headline TDNN's hidden layer: 250 columns of one image at three ascending row offsets, interleaved k-steps (48 of them)
static GemmDev Hidden(int off = 3, int col0 = 0, const ActImage *third = &kImgA) {
  GemmDev d = Base(250, true, true);
  Seg(&d, &kImgA, 256, col0, 250, -off);
  Seg(&d, &kImgA, 256, col0, 250, 0);
  Seg(&d, third, 256, col0, 250, off);
  d.interleave = 1;
  d.out_img = kImgB;
  return d;
}
static GemmDev First(uintptr_t src = 0x20000000) {      // float sources, W3 only, one per-utterance iVector segment
  GemmDev d = Base(250, true, false);
  for (int o = -1; o <= 1; o++) Seg(&d, nullptr, 40, 0, 40, o, 0, src);
  Seg(&d, nullptr, 100, 0, 100, 0, 1, 0x21000000);
  return d;
}
static GemmDev OneSeg(int n, int k, bool w3 = true) {      // one image-fed segment of k columns
  GemmDev d = Base(n, w3, w3);
  Seg(&d, w3 ? &kImgA : nullptr, (k + 3) / 4 * 4, 0, k, 0);
  return d;
}

struct Layer { const char *name; GemmDev d; };
static std::vector<Layer> Layers() {
  std::vector<Layer> v;
  v.push_back({"hidden", Hidden()});
  v.push_back({"first", First()});
  v.push_back({"output362", OneSeg(362, 250)});
  v.push_back({"lda40", OneSeg(40, 280, false)});
  v.push_back({"bottleneck128", OneSeg(128, 2048)});
  v.push_back({"wide1024", OneSeg(1024, 1024)});
  GemmDev r = Hidden();
  r.res = Fake<const float>(0x70000000); r.res_ld = 256; r.res_scale = 0.75f;
  v.push_back({"res", r});
  r.res_img = kImgA;
  v.push_back({"res_img", r});
  GemmDev m = Hidden();
  m.row_map = Fake<const int>(0x78000000);
  m.row_map_span128 = 150; m.row_map_span160 = 182;
  v.push_back({"map_fits", m});
  m.row_map_span160 = 224;
  v.push_back({"map_fits128", m});
  m.row_map_span128 = 200;
  v.push_back({"map_wide", m});
  m.row_map_span128 = 0; m.row_map_span160 = 0;
  v.push_back({"map_unknown", m});
  v.push_back({"far_offsets", Hidden(40)});                      // offsets 80 rows apart: no strip
  // one usability rule broken each
  v.push_back({"src_misaligned", First(0x20000004)});
  v.push_back({"col0_8", Hidden(3, 8)});
  v.push_back({"two_images", Hidden(3, 0, &kImgB)});
  v.push_back({"pad47", OneSeg(270, 250)});                      // 512-column tiles, 47 % padding
  v.push_back({"pad49_one_tile", OneSeg(130, 250)});             // one tile of >= 96 columns: taken unless RS_GEMM_B3_NARROW=0
  return v;
}

// ---------------------------------------------------------------------------------------------- switches
static const char *const kSwitchNames[] = {"B3", "B3I", "B3J", "B3J_WM", "B3J_SLOTS", "B3J_MR", "B3J_NARROW", "B3J_SMALL", "B3J_STRIP", "B3_NARROW", "CUS"};
static void SetSwitches(const std::string &spec) {      // "B3J=2,B3J_WM=1" or "-"
  for (const char *n : kSwitchNames) unsetenv((std::string("RS_GEMM_") + n).c_str());
  if (spec == "-") return;
  size_t at = 0;
  while (at < spec.size()) {
    const size_t end = std::min(spec.find(',', at), spec.size()), eq = spec.find('=', at);
    CHECK(eq < end, "switch spec %s", spec.c_str());
    setenv(("RS_GEMM_" + spec.substr(at, eq - at)).c_str(), spec.substr(eq + 1, end - eq - 1).c_str(), 1);
    at = end + 1;
  }
}

// ---------------------------------------------------------------------------------------------- the kernels' block decoding, restated
#ifndef GEMM_LAUNCH_RECORD
static void CheckCoverage(const GemmLaunch &p, const GemmDev &d, int rows, const char *what) {
  const int BM = p.bm(), SBM = p.small_bm(), ncol = (d.n + p.bn() - 1) / p.bn();
  std::vector<std::vector<std::pair<int, int>>> owned(ncol);
  const bool alt = p.nfirst < 0, three_ranges = p.family == GemmLaunch::kB3J;
  const int nfirst = std::abs(p.nfirst);
  CHECK(three_ranges || nfirst == 0, "%s: nfirst on a kernel without the range", what);
  CHECK(p.family != GemmLaunch::kExact || p.nbig == (rows + BM - 1) / BM, "%s: exact kernels take all row tiles full-height", what);
  const int big_blocks = (p.nbig + 7) / 8 * 8 * ncol, first_blocks = p.mixed ? (nfirst + 7) / 8 * 8 * ncol : 0;
  for (int b = 0; b < p.blocks; b++) {
    bool small;
    int bid;
    if (!p.mixed) { small = false; bid = b; }
    else if (!alt) {
      small = b < first_blocks || b >= first_blocks + big_blocks;
      bid = small ? (b < first_blocks ? b : b - big_blocks) : b - first_blocks;
    } else {
      const int gsz = 8 * ncol;
      if (b < 2 * first_blocks) {
        const int grp = b / gsz, within = b % gsz;
        small = (grp & 1) == 0;
        bid = (grp >> 1) * gsz + within;
      } else {
        const int b2 = b - 2 * first_blocks, big_left = big_blocks - first_blocks;
        small = b2 >= big_left;
        bid = first_blocks + (small ? b2 - big_left : b2);
      }
    }
    const int xcd = bid & 7, local = bid >> 3;
    const int rt = (local / ncol) * 8 + xcd, ct = local % ncol;
    const int row0 = small ? p.nbig * BM + rt * SBM : rt * BM;
    if (small ? row0 >= rows : rt >= p.nbig) continue;
    CHECK(row0 < rows, "%s: block %d starts at row %d of %d", what, b, row0, rows);
    owned[ct].push_back({row0, std::min(row0 + (small ? SBM : BM), rows)});
  }
  for (int ct = 0; ct < ncol; ct++) {
    std::sort(owned[ct].begin(), owned[ct].end());
    int at = 0;
    for (auto &r : owned[ct]) {
      CHECK(r.first == at, "%s: column tile %d: rows [%d, %d) follow row %d", what, ct, r.first, r.second, at);
      at = r.second;
    }
    CHECK(at == rows, "%s: column tile %d: rows from %d on have no block", what, ct, at);
  }
}
#endif

static void Case(const Layer &l, int rows, int share, int exclusive, const char *switches) {
  GemmDev d = l.d;
  d.share = share;
  d.exclusive = exclusive;
  SetSwitches(switches);
  char what[160], dec[200];
  std::snprintf(what, sizeof(what), "%s %d s%d x%d %s", l.name, rows, share, exclusive, switches);
#ifdef GEMM_LAUNCH_RECORD
  g_rec[0] = 0; g_res = 0;
  LaunchGemm(d, rows, nullptr, nullptr);
  std::snprintf(dec, sizeof(dec), "%s res=%d", g_rec, g_res);
  const bool img = GemmWritesImage(d);
#else
  const GemmSwitches sw = ReadGemmSwitches();
  const GemmLaunch p = PlanGemmLaunch(d, rows, 256, sw);
  DescribeGemmLaunch(p, dec, sizeof(dec));
  const bool img = GemmWritesImage(d, sw);
  CHECK(img == p.writes_image, "%s: GemmWritesImage and the plan disagree", what);
  CHECK(!p.residual_pass || d.res, "%s: a residual pass without a residual", what);
  CheckCoverage(p, d, rows, what);
#endif
  std::printf("%s | %s img=%d\n", what, dec, (int)img);
}

#ifndef GEMM_LAUNCH_RECORD
// One descriptor: "key=value" tokens in any order, then "name=" and the op's name up to the end of the line (it may hold blanks).
//   rows cu switches(as SetSwitches takes them)  n w3 w3i interleave share exclusive write_f32 out_img res(0 none, 1 floats, 2 operand image)
//   map(0 | 1) span128 span160  segs=<img 0|1>:<ld>:<col0>:<ncols>:<row_off>:<per_utt>:<source misaligned 0|1>;...
static long Field(const std::string &line, const char *key, long unset) {
  const std::string k = std::string(" ") + key + "=";
  const size_t at = (" " + line).find(k);
  return at == std::string::npos ? unset : std::atol(line.c_str() + at + k.size() - 1);
}
static std::string Text(const std::string &line, const char *key, bool to_end) {
  const std::string k = std::string(" ") + key + "=", l = " " + line;
  const size_t at = l.find(k);
  CHECK(at != std::string::npos, "descriptor without %s: %s", key, line.c_str());
  const size_t from = at + k.size(), end = to_end ? std::string::npos : l.find(' ', from);
  return l.substr(from, end == std::string::npos ? std::string::npos : end - from);
}
static void DescriptorCase(const std::string &line) {
  const int n = (int)Field(line, "n", 0), rows = (int)Field(line, "rows", 0), cu = (int)Field(line, "cu", 256);
  CHECK(n > 0 && rows > 0 && cu > 0, "descriptor: %s", line.c_str());
  GemmDev d = Base(n, Field(line, "w3", 0) != 0, Field(line, "w3i", 0) != 0);
  const std::string segs = Text(line, "segs", false);
  for (size_t at = 0; at < segs.size();) {
    const size_t end = std::min(segs.find(';', at), segs.size());
    long v[7] = {0, 0, 0, 0, 0, 0, 0};
    CHECK(std::sscanf(segs.substr(at, end - at).c_str(), "%ld:%ld:%ld:%ld:%ld:%ld:%ld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7, "segment in %s", line.c_str());
    CHECK(d.nsegs < (int)(sizeof(d.segs) / sizeof(d.segs[0])), "too many segments: %s", line.c_str());
    Seg(&d, v[0] ? &kImgA : nullptr, (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] ? 0x20000004 : 0x20000000);
    at = end + 1;
  }
  CHECK(d.nsegs > 0, "no segment: %s", line.c_str());
  d.interleave = (int)Field(line, "interleave", 0);
  d.share = (int)Field(line, "share", 1);
  d.exclusive = (int)Field(line, "exclusive", 0);
  d.write_f32 = (int)Field(line, "write_f32", 1);
  if (Field(line, "out_img", 0)) d.out_img = kImgB;
  const long res = Field(line, "res", 0);
  if (res) { d.res = Fake<const float>(0x70000000); d.res_ld = 256; d.res_scale = 0.66f; }
  if (res == 2) d.res_img = kImgA;
  if (Field(line, "map", 0)) {
    d.row_map = Fake<const int>(0x78000000);
    d.row_map_span128 = (int)Field(line, "span128", 0); d.row_map_span160 = (int)Field(line, "span160", 0);
  }
  SetSwitches(Text(line, "switches", false));
  const GemmSwitches sw = ReadGemmSwitches();
  const std::string name = Text(line, "name", true);
  const GemmLaunch p = PlanGemmLaunch(d, rows, GemmPlanCus(sw, cu), sw);
  CHECK(GemmWritesImage(d, sw) == p.writes_image, "%s: GemmWritesImage and the plan disagree", line.c_str());
  CHECK(!p.residual_pass || d.res, "%s: a residual pass without a residual", line.c_str());
  CheckCoverage(p, d, rows, line.c_str());
  char out[400];
  std::printf("gemm_launch: %s\n", DescribeGemmLaunchLine(name.c_str(), d, rows, p, out, sizeof(out)));
}
#endif

int main(int argc, char **argv) {
#ifndef GEMM_LAUNCH_RECORD
  if (argc > 1) {
    FILE *f = std::fopen(argv[1], "r");
    CHECK(f != nullptr, "cannot read %s", argv[1]);
    char buf[2048];
    while (std::fgets(buf, sizeof(buf), f)) {
      std::string line(buf);
      while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
      if (!line.empty() && line[0] != '#') DescriptorCase(line);
    }
    std::fclose(f);
    return 0;
  }
#else
  (void)argc; (void)argv;
#endif
  const std::vector<Layer> layers = Layers();
  const int all_rows[] = {1, 31, 32, 33, 127, 128, 129, 159, 160, 161, 1024, 4096, 4097, 8192, 8193, 8194, 16384, 16385, 16386, 81920, 81921, 83968};
  const int some_rows[] = {33, 4096, 8192, 8193, 81920, 81921};
  const int few_rows[] = {33, 4096, 16385, 81920, 81921};
  // the shipped switches: every layer, every row count
  for (const Layer &l : layers) {
    for (int rows : all_rows) Case(l, rows, 1, 0, "-");
    for (int rows : some_rows) Case(l, rows, 2, 0, "-");
  }
  // several decode pipelines in flight: the CU-exclusive form of the layers that run on GemmKernelB3
  for (const char *name : {"first", "col0_8"})
    for (const Layer &l : layers)
      if (!std::strcmp(l.name, name))
        for (int share : {1, 2})
          for (int rows : all_rows) Case(l, rows, share, 1, "-");
  // the switches the tests flip, alone and in the tests' combinations
  const char *const switch_sets[] = {
      "B3=0", "B3I=0", "B3J=0", "B3J=2", "B3J=2,B3J_WM=1,B3J_SLOTS=48", "B3J=2,B3J_WM=1,B3J_SLOTS=100000", "B3J=2,B3J_WM=2,B3J_SLOTS=48",
      "B3J=2,B3J_WM=2,B3J_SLOTS=100000", "B3J_WM=2", "B3J_MR=4", "B3J_MR=5", "B3J=2,B3J_MR=4", "B3J=2,B3J_MR=5", "B3J_NARROW=0", "B3J_SLOTS=24",
      "B3J_NARROW=0,B3J_SLOTS=24", "B3J_SMALL=0", "B3J_STRIP=0", "B3_NARROW=0"};
  const char *const switch_layers[] = {"hidden", "first", "output362", "lda40", "bottleneck128", "wide1024", "res", "res_img", "map_wide", "pad49_one_tile"};
  for (const char *sw : switch_sets)
    for (const char *name : switch_layers)
      for (const Layer &l : layers)
        if (!std::strcmp(l.name, name))
          for (int rows : few_rows) Case(l, rows, 1, 0, sw);
#ifndef GEMM_LAUNCH_RECORD
  // the alternating block order (RS_GEMM_B3J_STAGGER=2, a measurement switch the shipped build does not read): coverage only
  SetSwitches("-");
  GemmSwitches alt = ReadGemmSwitches();
  alt.b3j_stagger = 2;
  int alternating = 0;
  for (const Layer &l : layers)
    for (int rows : all_rows) {
      const GemmLaunch p = PlanGemmLaunch(l.d, rows, 256, alt);
      CheckCoverage(p, l.d, rows, l.name);
      alternating += p.nfirst < 0;
    }
  CHECK(alternating > 0, "no launch of the sweep alternates");
#endif
  return 0;
}
