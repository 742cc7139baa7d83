// The base-feature kernel, one wave per frame: MfccKernel (RS_FEAT_FBANK 0) and FbankKernel (RS_FEAT_FBANK 1), included twice by
// feat_kernels.hip like online_cmvn_kernel.inc.  Steps 1-4 -- load, dither, DC removal, pre-emphasis, window, split-radix FFT, power
// spectrum -- are one text for both, the same float operations on the same operands; what follows the power spectrum is the type's
// own: mel + log + DCT + lifter (feat/feature-mfcc.cc:28-80), or the log-mel filterbank row itself (feat/feature-fbank.cc:72-123).
// A preprocessor switch and not a template parameter or a shared __device__ front: with either of those the compiler allocated
// MfccKernel's registers differently (profiles/micro/mfcc_isa_diff.sh); with this its instantiations are the code they were.
//
// WPB = waves (frames) per workgroup.  4 by default; 16 with all the CU's LDS requested when several decode pipelines are in
// flight, so that no GemmKernelB3 workgroup of another pipeline can share the CU (DESIGN.md section 5: that kernel
// perturbs this one's LDS-staged arithmetic when they share a CU).
// TAB: the FFT plan's records (21.5 KB for a 512-point window) are copied into LDS once per workgroup and every wave reads its records
// from there: 21 of a frame's ~60 vector memory requests become 1.3 (WPB = 16), and it is their number the kernel is bound by.
template <int NFFT, int WPB, bool TAB = false>   // padded window (real points)
#if RS_FEAT_FBANK
__global__ __launch_bounds__(64 * WPB) void FbankKernel(MfccDev m, FbankDev f, BatchGeom g, const int16_t *__restrict__ pcm,
                                                        float *__restrict__ feats, int ld, const int *__restrict__ out_rows) {
#else
__global__ __launch_bounds__(64 * WPB) void MfccKernel(MfccDev m, BatchGeom g, const int16_t *__restrict__ pcm,
                                                       float *__restrict__ feats, int ld, const int *__restrict__ out_rows) {
#endif
  constexpr int NC = NFFT / 2;        // complex points
  const int4 *tasks = reinterpret_cast<const int4 *>(m.fft_tasks);
  const float *fft_tw = m.fft_tw;
  extern __shared__ __attribute__((aligned(16))) float mfcc_lds[];
  float (*xrb)[NC] = reinterpret_cast<float (*)[NC]>(mfcc_lds);
  float (*xib)[NC] = reinterpret_cast<float (*)[NC]>(mfcc_lds + WPB * NC);
  float (*pw)[NC + 1] = reinterpret_cast<float (*)[NC + 1]>(mfcc_lds + WPB * (2 * NC));
#if RS_FEAT_FBANK
  constexpr int kLm = 0;          // (no slab of log mel energies: they go straight into the row)
#else
  constexpr int kLm = 64;
  float (*lm)[64] = reinterpret_cast<float (*)[64]>(mfcc_lds + WPB * (3 * NC + 1));
#endif
  // (the wave number through readfirstlane: the row, its utterance, frame, sample and noise addresses are then scalars -- s_load look-ups,
  // one address register per request instead of a 64-bit vector addition each; the front end was 350 of the kernel's ~1 000 vector
  // instructions per frame, and the kernel is bound by their number)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float4 *lrec = reinterpret_cast<float4 *>(mfcc_lds + WPB * (3 * NC + 1 + kLm));      // TAB: [level][3][64] float4
  if (TAB) {
    const int n4 = m.fft_num_levels * 64 * 3;
    for (int i = threadIdx.x; i < n4; i += 64 * WPB) {
      const int rec = i / 3, c = i - 3 * rec;
      lrec[((rec >> 6) * 3 + c) * 64 + (rec & 63)] = m.fft_recs[i];
    }
    __syncthreads();
  }
  const int row = blockIdx.x * WPB + wave;
  const bool active = row < g.total_rows;
  // What does not depend on the frame is requested first, ahead of the row's own chain of look-ups (row -> utterance -> offsets ->
  // samples): the first FFT level's record here, the post-processing pass's gather indices and factors and the lane's mel filter and
  // lifter in front of the FFT, whose seven LDS round trips cover them.
  // The kernel is a chain of ~20 dependent trips to L2 per frame, and eight waves per SIMD -- all it can hold -- do not hide them
  // (its LDS pipe is half busy since the swizzle, its vector ALU 63 %: profiles/micro/pmc_lds.sh, pmc_inst.sh; round 6).
  constexpr bool kFast = NFFT == 512 || NFFT == 256;      // one pre-addressed record per lane and level, fft_post rounds of 64 lanes
  constexpr int kPostRounds = NFFT / 256;                 // k = 1 .. NFFT / 4 of the post-processing pass: two rounds at 512, one at 256
  float4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
  const bool recs_on = kFast && m.fft_recs != nullptr;
  if (recs_on && !TAB) {
    const char *lv = reinterpret_cast<const char *>(m.fft_recs) + (unsigned)lane * 48u;
    a0 = *reinterpret_cast<const float4 *>(lv); a1 = *reinterpret_cast<const float4 *>(lv + 16); a2 = *reinterpret_cast<const float4 *>(lv + 32);
  }

  int u = 0, t = 0;
  bool first = false, last = false;      // this row is the utterance's frame 0 / frame T - 1: its cepstra are also the left / right halo rows'
  if (active) {
    u = g.d_row_utt[row];
    t = g.d_row_t[row];
    const int T = g.d_num_frames[u];
    // A halo row repeats the edge frame next to it: the wave of that frame writes the copies, the halo rows' own waves have
    // nothing to do (9 % of the rows of a batch of 3 s utterances).  No workgroup-wide step anywhere below: a wave may leave.
    if (T > 0 && (t < 0 || t >= T)) return;
    first = T > 0 && t == 0;
    last = T > 0 && t == T - 1;
    t = t >= T ? T - 1 : t;
    t = t < 0 ? 0 : t;          // (the halo rows of an utterance too short for one frame: frame 0 of whatever follows it, never read back)
  }
#ifdef RS_MFCC_PROFILE
  long long mp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mt = clock64();
#define RS_MT(i) do { const long long n_ = clock64(); mp[i] += n_ - mt; mt = n_; } while (0)
#else
#define RS_MT(i) do { } while (0)
#endif
  float raw_energy = 0.f;
  float *xr = xrb[wave], *xi = xib[wave];
  if (active) {
    const int16_t *src = pcm + g.d_sample_off[u] + (int64_t)t * m.shift;
    // 1. load (int16 -> float, unscaled), dither, DC removal.  The frame sum follows the reference's BLAS call
    // (VectorBase::Sum() = cblas_sdot(n, x, 1, &one, 0), OpenBLAS kernel/x86_64/sdot.c strided loop): adjacent pairs are added
    // in float and the pair sums accumulated in a double.  With integer samples every order gives the same sum; with the
    // dither noise in, a differently rounded mean re-rounds every sample of a loud frame and moves the cepstra by 1e-3.  The
    // double accumulation is a wave reduction here: the pair sums of a frame span far fewer than 53 bits, so it is exact in
    // any order (it would take a pair cancelling to below 2^-33 of the frame's peak to make the order matter).
    double dsum = 0.0;
    // (dither off: finite stand-ins multiplied by 0 -- v + 0 is v -- so that the loads below carry no condition: written as
    // `if (noise) v += ...` the compiler put every load under a branch with a full wait behind it, 16 dependent round trips per frame)
    const float *noise = m.dither ? m.dither + (size_t)(t + (g.d_frame0 ? g.d_frame0[u] : 0)) * m.win : m.window;
    const float dv = m.dither ? m.dither_value : 0.f;
    constexpr int JP = NFFT / 128;                      // sample pairs per lane
    float s0[JP], s1[JP], n0[JP], n1[JP], w0[JP], w1[JP];
    // A lane's two samples, noise values and window values are neighbours: with an even window and aligned rows (the usual case: a
    // wave-uniform test) each pair is ONE request -- 12 per frame instead of 24.  The kernel's texture addresser is busy 89 % of the
    // launch (profiles/micro/pmc_ta.sh): ~80 vector memory requests per frame at 16 cycles each are what a frame costs a CU.
    const bool pairs = (m.win & 1) == 0 && m.win >= 2 && ((reinterpret_cast<uintptr_t>(src) & 3) == 0) &&
                       ((reinterpret_cast<uintptr_t>(noise) & 7) == 0) && ((reinterpret_cast<uintptr_t>(m.window) & 7) == 0);
    if (pairs) {
#pragma unroll
      for (int j = 0; j < JP; j++) {
        const int pi = lane + RS_WAVE * j, pc = 2 * pi < m.win ? pi : (m.win >> 1) - 1;      // pair index, clamped into the window
        const unsigned b = (unsigned)pc;
        const int sp = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(src) + 4u * b);
        const float2 np = *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(noise) + 8u * b);
        const float2 wp = *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(m.window) + 8u * b);
        s0[j] = (float)(short)(sp & 0xffff); s1[j] = (float)(sp >> 16);
        n0[j] = np.x; n1[j] = np.y;
        w0[j] = wp.x; w1[j] = wp.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < JP; j++) {                      // all requests first ...
        const int i0 = 2 * (lane + RS_WAVE * j), c0 = i0 < m.win ? i0 : m.win - 1, c1 = i0 + 1 < m.win ? i0 + 1 : m.win - 1;
        // (scalar base + 32-bit lane offset: the addressing mode that costs no vector instruction per request)
        const unsigned b0 = (unsigned)c0, b1 = (unsigned)c1;
        s0[j] = (float)*reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(src) + 2u * b0);
        s1[j] = (float)*reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(src) + 2u * b1);
        n0[j] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(noise) + 4u * b0);
        n1[j] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(noise) + 4u * b1);
        w0[j] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(m.window) + 4u * b0);
        w1[j] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(m.window) + 4u * b1);
      }
    }
    float v0[JP], v1[JP];
#pragma unroll
    for (int j = 0; j < JP; j++) {                      // ... then Dither(): data[i] += RandGauss(&rstate) * dither_value (no FMA: -ffp-contract=off)
      const int i0 = 2 * (lane + RS_WAVE * j), i1 = i0 + 1;
      v0[j] = s0[j] + n0[j] * dv; v1[j] = s1[j] + n1[j] * dv;
      if (i1 < m.win) dsum += (double)(v0[j] + v1[j]);
      else if (i0 < m.win) dsum += (double)v0[j];
    }
    dsum = WaveSumF64(dsum);      // (exact in any order, see above: row rotations + four readlanes instead of six ds_bpermute pairs)
    // DC removal (x[i] += -mean), then
    // 2. pre-emphasis (uses the *un-emphasised* left neighbour, as the backwards loop of the reference does) and window; the even /
    // odd samples are the real / imaginary parts of the half-length complex transform.  A lane keeps its sample pairs in registers
    // from the load to here: the odd sample's left neighbour is the pair's even one, the even sample's is the previous lane's odd one
    // (one cross-lane move per pair).  Through an LDS copy of the frame -- written in pairs, read back sample by sample with the
    // window value fetched under the same condition -- this step was 200 of the kernel's 1 300 instructions per frame, and the
    // kernel is bound by their number (round 6).  Same subtractions and products on the same operands.
    const float dc = m.remove_dc ? (float)dsum / (float)m.win : 0.f;      // (x - 0.f is x)
    float e_raw = 0.f, e_win = 0.f;
#pragma unroll
    for (int j = 0; j < JP; j++) {
      const int i0 = 2 * (lane + RS_WAVE * j), i1 = i0 + 1;
      float left = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v1[j]), 0x138, 0xF, 0xF, false));      // wave_shr:1 -- lane l - 1's odd sample
      const float carry = j > 0 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v1[j > 0 ? j - 1 : 0]), RS_WAVE - 1)) : v0[0];      // lane 0: the previous round's last sample; sample 0 is its own neighbour
      left = lane == 0 ? carry : left;
      const float c0 = v0[j] - dc, c1 = v1[j] - dc, p0 = left - dc;
      const float y0 = i0 < m.win ? (c0 - m.preemph * p0) * w0[j] : 0.f;
      const float y1 = i1 < m.win ? (c1 - m.preemph * c0) * w1[j] : 0.f;
      if (m.use_energy) {      // (kernel-uniform)
        e_raw += (i0 < m.win ? c0 * c0 : 0.f) + (i1 < m.win ? c1 * c1 : 0.f);
        e_win += y0 * y0 + y1 * y1;
      }
      // (point i of the half-length transform lives at i ^ g(i >> 5), g linear in the three bits: MfccDev::fft_swz, zero without the
      // pre-addressed plan; i = lane + 64 j, so bit 5 is the lane's and bits 6, 7 are j's)
      const int pos = ((lane ^ ((lane & 32) ? m.fft_swz[0] : 0)) ^ ((j & 1) ? m.fft_swz[1] : 0) ^ ((j & 2) ? m.fft_swz[2] : 0)) + RS_WAVE * j;
      xr[pos] = y0;
      xi[pos] = y1;
    }
    if (m.use_energy) raw_energy = logf(fmaxf(WaveSum(m.raw_energy ? e_raw : e_win), FLT_EPSILON));
  }
  RS_MT(0);
  WaveLdsSync();
  RS_MT(1);
  // (requested here, where the registers of the sample pairs are free again; first used seven LDS round trips later)
  int pp_k[2] = {0, 0}, pp_d[2] = {0, 0};
  float pp_re[2] = {0.f, 0.f}, pp_im[2] = {0.f, 0.f};
  if (kFast) {
#pragma unroll
    for (int q = 0; q < kPostRounds; q++) {
      const int k = lane + 1 + RS_WAVE * q;          // (2 k <= NFFT / 2 for both)
      (void)k;
      const float4 pr = m.fft_post[q * RS_WAVE + lane];      // (one request instead of four: the kernel is bound by the NUMBER of its vector memory requests)
      pp_k[q] = __float_as_int(pr.x); pp_d[q] = __float_as_int(pr.y);
      pp_re[q] = pr.z; pp_im[q] = pr.w;
    }
  }
#if RS_FEAT_FBANK
  const int4 mrec = m.mel_rec[lane < m.nbins ? lane : 0], mrec_hi = m.mel_rec[lane + RS_WAVE < m.nbins ? lane + RS_WAVE : 0];      // the lane's filters: bins lane, 64 + lane
#else
  const int mlane = lane < m.nbins ? lane : 0, clane = lane < m.nceps ? lane : 0;
  const int4 mrec = m.mel_rec[mlane];
  const int mel_off = mrec.x, mel_n = mrec.y, mel_s = mrec.z;
  const float lift = m.lifter[clane];
#endif
  // 3. split-radix complex FFT, level by level (tasks of one level touch disjoint points)
  if (kFast && m.fft_recs) {
    // at most one task per lane and level: the record of the NEXT level (task + its twiddle factors, three 16-byte loads of one
    // 48-byte record) is requested before the current level runs, so no level waits for a global round trip -- the task-then-twiddles
    // pair of dependent loads per level was 14 of the frame's ~45 (profiles/r04/mfcc_notes.txt).  Round 6: 64 records per level (a
    // lane's record at a fixed offset from the level's base), the points' LDS offsets in the record, two register sets in turn.
    const int nl = m.fft_num_levels;
    const int xi_off = (int)(xi - xr);
    const char *rec0 = reinterpret_cast<const char *>(m.fft_recs);
    const unsigned lane_off = (unsigned)lane * 48u;
    float4 b0, b1, b2;
#define RS_FFT_FETCH(L, r0, r1, r2)                                                              \
    {                                                                                            \
      if (TAB) {                                                                                 \
        r0 = lrec[((L) * 3 + 0) * 64 + lane]; r1 = lrec[((L) * 3 + 1) * 64 + lane]; r2 = lrec[((L) * 3 + 2) * 64 + lane]; \
      } else {                                                                                   \
        const char *lv = rec0 + (size_t)(L) * (64 * 48);                                         \
        r0 = *reinterpret_cast<const float4 *>(lv + lane_off);                                   \
        r1 = *reinterpret_cast<const float4 *>(lv + lane_off + 16);                              \
        r2 = *reinterpret_cast<const float4 *>(lv + lane_off + 32);                              \
      }                                                                                          \
    }
    if (TAB) RS_FFT_FETCH(0, a0, a1, a2)
    for (int L = 0; L < nl; L += 2) {      // (level 0's record: requested at the top of the kernel)
      if (L + 1 < nl) RS_FFT_FETCH(L + 1, b0, b1, b2)
      if (active) SrfftRunRec(a0, a1, a2, xr, xi_off);
      WaveLdsSync();
      if (L + 1 >= nl) break;
      if (L + 2 < nl) RS_FFT_FETCH(L + 2, a0, a1, a2)
      if (active) SrfftRunRec(b0, b1, b2, xr, xi_off);
      WaveLdsSync();
    }
#undef RS_FFT_FETCH
  } else {
    for (int L = 0; L < m.fft_num_levels; L++) {
      if (active)
        for (int ti = m.fft_level_begin[L] + lane; ti < m.fft_level_begin[L + 1]; ti += RS_WAVE) SrfftRunTask(tasks[ti], fft_tw, xr, xi);
      WaveLdsSync();
    }
  }
  RS_MT(2);
  // 4. real-FFT post-processing (srfft.cc:379-417) fused with the power spectrum (feature-functions.cc:41-49);
  // spectrum element k of the bit-reversal pass is element perm[k] of the in-place result
  if (active) {
    auto post = [&](int k, int pk, int pd, float kn_re, float kn_im) __attribute__((always_inline)) {
      const int kd = NC - k;
      const float bk_re = xr[pk], bk_im = xi[pk], bd_re = xr[pd], bd_im = xi[pd];
      const float ck_re = 0.5f * (bk_re + bd_re), ck_im = 0.5f * (bk_im - bd_im);
      const float dk_re = 0.5f * (bk_im + bd_im), dk_im = -0.5f * (bk_re - bd_re);
      // A_k = C_k + kN D_k
      const float a_re = ck_re + (kn_re * dk_re - kn_im * dk_im);
      const float a_im = ck_im + (kn_re * dk_im + kn_im * dk_re);
      pw[wave][k] = a_re * a_re + a_im * a_im;
      if (kd != k) {
        // A_k' = conj(C_k) + (-conj(kN)) conj(D_k)
        const float nd_im = -dk_im, nk_re = -kn_re;
        const float b_re = ck_re + (nk_re * dk_re - kn_im * nd_im);
        const float b_im = -ck_im + (nk_re * nd_im + kn_im * dk_re);
        pw[wave][kd] = b_re * b_re + b_im * b_im;
      }
    };
    if (kFast) {
#pragma unroll
      for (int q = 0; q < kPostRounds; q++) post(lane + 1 + RS_WAVE * q, pp_k[q], pp_d[q], pp_re[q], pp_im[q]);
    } else {
      for (int k = lane + 1; 2 * k <= NC; k += RS_WAVE) post(k, m.fft_perm[k], m.fft_perm[NC - k], m.fft_kn[2 * k], m.fft_kn[2 * k + 1]);
    }
    if (lane == 0) {
      const float d0 = xr[m.fft_perm[0]], d1 = xi[m.fft_perm[0]];
      const float zeroth = d0 + d1, n2th = d0 - d1;
      pw[wave][0] = zeroth * zeroth;
      pw[wave][NC] = n2th * n2th;
    }
  }
  WaveLdsSync();
  RS_MT(3);
#if RS_FEAT_FBANK
  // 5. --use-power=false: the magnitude spectrum (feature-fbank.cc:99-100; VectorBase::ApplyPow(0.5) is sqrt) ...
  if (!f.use_power) {
    if (active)
      for (int k = lane; k <= NC; k += RS_WAVE) pw[wave][k] = sqrtf(pw[wave][k]);
    WaveLdsSync();
  }
  // ... then per mel bin the dot product, the floor and the log (feature-fbank.cc:108-113), straight into the row -- one bin per lane, a
  // second pass of lanes for bins 64-127 -- and the energy into its column (:116-122).  Every column written is below
  // nbins + (use_energy ? 1 : 0), the row's width, which the leading dimension covers.
  if (active) {
    auto store = [&](int col, float v) __attribute__((always_inline)) {
      feats[(size_t)(out_rows ? out_rows[row] : row) * ld + col] = v;      // out_rows: streams write into their pool rows
      if (first) for (int k = 1; k <= g.L; k++) feats[(size_t)(out_rows ? out_rows[row - k] : row - k) * ld + col] = v;
      if (last) for (int k = 1; k <= g.R; k++) feats[(size_t)(out_rows ? out_rows[row + k] : row + k) * ld + col] = v;
    };
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const int bin = lane + RS_WAVE * p;
      if (bin >= m.nbins) continue;
      const int4 r = p ? mrec_hi : mrec;      // {first FFT bin, length, offset of the weights}
      const float *w = m.mel_weights + r.z;
      float e = 0.f;
      for (int i = 0; i < r.y; i++) e += w[i] * pw[wave][r.x + i];
      if (f.use_log) e = logf(fmaxf(e, FLT_EPSILON));
      store(f.mel_col0 + bin, e);
    }
    if (m.use_energy && lane == 0) store(f.energy_col, fmaxf(raw_energy, m.log_energy_floor));
  }
  RS_MT(4);
#else
  // 5. mel filterbank + log
  if (active && lane < m.nbins) {
    const int off = mel_off, len = mel_n;
    const float *w = m.mel_weights + mel_s;
    float e = 0.f;
    for (int i = 0; i < len; i++) e += w[i] * pw[wave][off + i];
    lm[wave][lane] = logf(fmaxf(e, FLT_EPSILON));
  }
  WaveLdsSync();
  RS_MT(4);
  // 6. DCT + lifter, write the row
  if (active && lane < m.nceps) {
    const float *d = m.dct + lane * m.nbins;
    float c = 0.f;
    for (int b = 0; b < m.nbins; b++) c += d[b] * lm[wave][b];
    c *= lift;
    if (m.use_energy && lane == 0) c = fmaxf(raw_energy, m.log_energy_floor);
    feats[(size_t)(out_rows ? out_rows[row] : row) * ld + lane] = c;      // out_rows: streams write into their pool rows
    if (first) for (int k = 1; k <= g.L; k++) feats[(size_t)(out_rows ? out_rows[row - k] : row - k) * ld + lane] = c;
    if (last) for (int k = 1; k <= g.R; k++) feats[(size_t)(out_rows ? out_rows[row + k] : row + k) * ld + lane] = c;
  }
  RS_MT(5);
#endif
#ifdef RS_MFCC_PROFILE
  if (lane == 0 && row % 9973 == 0)
    printf("mfcc row %d: load+dc %lld preemph+window %lld fft %lld power %lld mel %lld dct %lld\n", row, mp[0], mp[1], mp[2], mp[3], mp[4], mp[5]);
#endif
#undef RS_MT
}

