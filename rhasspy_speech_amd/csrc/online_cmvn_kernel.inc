// The online CMVN kernel's text (feat_kernels.hip includes it twice): RS_CMVN_SPK 0 = OnlineCmvnKernel, the kernel of every stream
// and batch without speaker statistics, whose text -- and so whose code -- is what it was before the speaker term existed; RS_CMVN_SPK 1
// = OnlineCmvnSpkKernel, with SmoothOnlineCmvnStats' speaker term (online-feature.cc:393-404): the speaker's sums are added before
// the global ones.  spk holds (D + 1) doubles per slot -- the carried sums and their count -- and spk_slot[u] is the slot of
// utterance u, or -1 for a stream without speaker statistics, whose arithmetic is then the plain kernel's.
#if RS_CMVN_SPK
#define RS_CMVN_KERNEL OnlineCmvnSpkKernel
#else
#define RS_CMVN_KERNEL OnlineCmvnKernel
#endif
template <int kPer>      // elements of a chunk per thread, at most: kCmvnTC * D <= 256 * kPer
__global__ __launch_bounds__(256) void RS_CMVN_KERNEL(CmvnDev c, BatchGeom g, const float *__restrict__ in, float *__restrict__ out, int ld,
                                                        const int *__restrict__ t_begin, double *__restrict__ state, const int *__restrict__ state_slot
#if RS_CMVN_SPK
                                                        , const double *__restrict__ spk, const int *__restrict__ spk_slot
#endif
                                                        ) {
  // LDS by the feature dimension (40: 23 KB; as [32][128] arrays the kernel held 68 KB of a CU, i.e. the place of one of the two
  // layer-GEMM workgroups of the call in flight beside it), and the NEXT chunk's frames are in flight, in registers, while a chunk
  // is processed (every chunk used to start with a trip to memory: ten of them per 3 s utterance).
  extern __shared__ __attribute__((aligned(16))) unsigned char cmvn_smem[];
  const int u = blockIdx.x, tid = threadIdx.x, D = c.dim, W = c.cmn_window;
  double *ss = reinterpret_cast<double *>(cmvn_smem);                 // [TC][D] running sums after each frame
  double *gs = ss + kCmvnTC * D;                                       // [D] global stats (read per element in step 3 while the window is not full)
  double *nn = gs + D, *aa = nn + kCmvnTC;                             // [TC] frame count in the window; weight of the global stats
  float *xs = reinterpret_cast<float *>(aa + kCmvnTC);                // [TC][D] the chunk
  float *xp = xs + kCmvnTC * D;                                        // [TC][D] the frames leaving the window while the chunk enters
  float *al = xp + kCmvnTC * D;                                        // [TC] -1 / (smoothed count)
  float *edge = al + kCmvnTC;                                          // [2][D] normalised first / last frame (halo rows replicate them)
#if RS_CMVN_SPK
  double *sps = reinterpret_cast<double *>(edge + 2 * D);              // [D] speaker sums (the floats before them are an even number)
  double *bb = sps + D;                                                // [TC] weight of the speaker stats
  double scount = 0.0;                                                 // the speaker statistics' count (0: none)
  {
    const int sslot = spk_slot[u];
    if (sslot >= 0) {
      scount = spk[(size_t)(D + 1) * sslot + D];
      if (tid < D) sps[tid] = spk[(size_t)(D + 1) * sslot + tid];
    }
  }
#endif
  if (tid < D) gs[tid] = c.global_stats[tid];
  const int T = g.d_num_frames[u];
  const size_t base = (size_t)g.d_row_base[u] + g.L;
  double sum = 0.0, count = 0.0;                  // threads < D
  const double gcount = c.global_stats[D];
  const int t_first = t_begin ? t_begin[u] : 0;
  double *park = t_begin ? state + (size_t)(D + 1) * state_slot[u] : nullptr;
  if (park && t_first > 0 && tid < D) { sum = park[tid]; count = park[D]; }
  float nx[kPer], np[kPer];
  const int i_first = tid / D, d_first = tid - i_first * D, i_step = 256 / D, d_step = 256 - i_step * D;      // element tid + 256 q = (frame, dimension), by steps
  auto fetch = [&](int t0) {                             // element idx = tid + 256 q of the chunk that starts at frame t0
    const int n = T - t0 < kCmvnTC ? T - t0 : kCmvnTC;
    int i = i_first, d = d_first;
#pragma unroll
    for (int q = 0; q < kPer; q++) {
      // (no load under a condition: an element past the chunk's end re-reads the chunk's first frame, a frame that has no
      // predecessor W frames back reads frame 0; neither value is used)
      const int ti = t0 + (i < n ? i : 0), tp = ti - W > 0 ? ti - W : 0;
      nx[q] = in[(base + ti) * ld + d];
      np[q] = in[(base + tp) * ld + d];
      i += i_step; d += d_step;
      if (d >= D) { d -= D; i++; }
    }
  };
#ifdef RS_CMVN_PROFILE
  long long cp[6] = {0, 0, 0, 0, 0, 0}, ct = clock64();
#define RS_CT(i) do { const long long n_ = clock64(); cp[i] += n_ - ct; ct = n_; } while (0)
#else
#define RS_CT(i) do { } while (0)
#endif
  if (t_first < T) fetch(t_first);
  RS_CT(0);
  for (int t0 = t_first; t0 < T; t0 += kCmvnTC) {
    const int n = T - t0 < kCmvnTC ? T - t0 : kCmvnTC;
#pragma unroll
    for (int q = 0; q < kPer; q++) {
      const int idx = tid + 256 * q;
      // (every request is waited for HERE, used or not: one that is consumed under a condition stays "possibly in flight" for the
      // compiler, and the next fetch() into the same register then waits vmcnt(0) -- for this chunk's output stores as well)
      __asm__ volatile("" : "+v"(nx[q]), "+v"(np[q]));
      if (idx < n * D) { xs[idx] = nx[q]; xp[idx] = np[q]; }      // (xp is read where a frame leaves the window, nowhere else)
    }
    __syncthreads();
    RS_CT(1);
    if (t0 + kCmvnTC < T) fetch(t0 + kCmvnTC);
    if (tid < D) {
      if (n == kCmvnTC && (t0 >= W || t0 + kCmvnTC <= W)) {
        // A whole chunk whose frames all push an old frame out of the window, or none does: the chunk's values of this dimension
        // first (independent LDS reads, all in flight together), then the chain of additions in registers, then the running sums
        // back.  Read, add and write frame by frame, every frame waited out an LDS round trip behind the previous frame's write
        // (215 cycles per frame, 60 % of the kernel; round 6).  Same additions in the same order.
        float xv[kCmvnTC], pv[kCmvnTC];
        double sv[kCmvnTC];
        const bool leaving = t0 >= W;
#pragma unroll
        for (int i = 0; i < kCmvnTC; i++) xv[i] = xs[i * D + tid];
        if (leaving) {
#pragma unroll
          for (int i = 0; i < kCmvnTC; i++) pv[i] = xp[i * D + tid];
#pragma unroll
          for (int i = 0; i < kCmvnTC; i++) { sum += (double)xv[i]; sum -= (double)pv[i]; sv[i] = sum; }      // (count + 1 - 1)
          count += 1.0; count -= 1.0;
          if (tid == 0) {
#pragma unroll
            for (int i = 0; i < kCmvnTC; i++) nn[i] = count;
          }
        } else {
#pragma unroll
          for (int i = 0; i < kCmvnTC; i++) { sum += (double)xv[i]; sv[i] = sum; }
          if (tid == 0) {
#pragma unroll
            for (int i = 0; i < kCmvnTC; i++) nn[i] = count + (double)(i + 1);
          }
          count += (double)kCmvnTC;
        }
#pragma unroll
        for (int i = 0; i < kCmvnTC; i++) ss[i * D + tid] = sv[i];
      } else {
#pragma unroll 4
        for (int i = 0; i < n; i++) {
          sum += (double)xs[i * D + tid];
          count += 1.0;
          if (t0 + i - W >= 0) { sum -= (double)xp[i * D + tid]; count -= 1.0; }
          ss[i * D + tid] = sum;
          if (tid == 0) nn[i] = count;
        }
      }
    }
    __syncthreads();
    RS_CT(2);
    if (tid < n) {
      double nf = nn[tid], a = 0.0;
#if RS_CMVN_SPK
      {
        double b = 0.0;
        if (nf < (double)W && scount > 0.0) {
          double from_speaker = (double)W - nf;
          if (from_speaker > (double)c.speaker_frames) from_speaker = (double)c.speaker_frames;
          if (from_speaker > scount) from_speaker = scount;
          if (from_speaker > 0.0) { b = from_speaker / scount; nf += b * scount; }
        }
        bb[tid] = b;
      }
#endif
      if (nf < (double)W) {
        double from_global = (double)W - nf;
        if (from_global > (double)c.global_frames) from_global = (double)c.global_frames;
        if (from_global > 0.0) { a = from_global / gcount; nf += a * gcount; }
      }
      aa[tid] = a;
      al[tid] = (float)(-1.0 / nf);
    }
    __syncthreads();
    RS_CT(3);
    {
      // (element tid + 256 q by steps, as in fetch(): no division by the runtime dimension; the LDS reads of all of a thread's
      // elements before the arithmetic)
      int i = i_first, d = d_first;
      double svq[kPer], aq[kPer], gq[kPer];
#if RS_CMVN_SPK
      double bq[kPer], sq[kPer];
#endif
      float alq[kPer], xq[kPer];
      int iq[kPer], dq[kPer];
#pragma unroll
      for (int q = 0; q < kPer; q++) {
        iq[q] = i; dq[q] = d;
        const bool on = i < n;
        const int idx = on ? i * D + d : 0, ii = on ? i : 0;
        svq[q] = ss[idx]; aq[q] = aa[ii]; gq[q] = gs[d]; alq[q] = al[ii]; xq[q] = xs[idx];
#if RS_CMVN_SPK
        bq[q] = bb[ii]; sq[q] = scount > 0.0 ? sps[d] : 0.0;
#endif
        i += i_step; d += d_step;
        if (d >= D) { d -= D; i++; }
      }
#pragma unroll
      for (int q = 0; q < kPer; q++) {
        if (iq[q] < n) {
          double sv = svq[q];
#if RS_CMVN_SPK
          if (bq[q] > 0.0) sv += bq[q] * sq[q];
#endif
          if (aq[q] > 0.0) sv += aq[q] * gq[q];
          const float offset = (float)((double)alq[q] * sv);
          const float yv = xq[q] + offset;
          out[(base + t0 + iq[q]) * ld + dq[q]] = yv;
          if (t0 + iq[q] == 0) edge[dq[q]] = yv;
          if (t0 + iq[q] == T - 1) edge[D + dq[q]] = yv;
        }
      }
    }
    __syncthreads();
    RS_CT(4);
  }
#ifdef RS_CMVN_PROFILE
  if (tid == 0 && u % 61 == 0) printf("cmvn utt %d (T=%d): first fetch %lld | stage %lld walk %lld scalars %lld apply %lld\n", u, T, cp[0], cp[1], cp[2], cp[3], cp[4]);
#endif
#undef RS_CT
  if (park && tid < D) { park[tid] = sum; if (tid == 0) park[D] = count; }
  if (T > 0 && !t_begin) {
    for (int idx = tid; idx < g.L * D; idx += 256) out[(base - g.L + idx / D) * ld + idx % D] = edge[idx % D];
    for (int idx = tid; idx < g.R * D; idx += 256) out[(base + T + idx / D) * ld + idx % D] = edge[D + idx % D];
  }
}
#undef RS_CMVN_KERNEL
