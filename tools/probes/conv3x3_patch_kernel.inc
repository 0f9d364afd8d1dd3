// Retired from csrc/conv_split.hip: the register-staged 8-row 3x3 kernel (weight tile of a tap fetched into VGPRs, stashed to LDS, two
// barriers per tap).  conv3x3_patch_dma_kernel (same tiles, weight tiles by LDS-DMA two taps ahead, one barrier per tap) replaced it on
// every shape; it stayed reachable only behind a run-time switch (UNIGEN_CONV_DMA8=0) that nothing set.  It pasted into conv_split.hip
// after PatchArgs and was launched as conv3x3_patch_kernel<GN, 4> (128 output channels per workgroup) or <GN, 2> (64) with the grid
// and block of the DMA kernel.  Kept for the record only.
// NI: 16-channel output blocks per wave.  4 = 128 output channels per workgroup; 2 = 64 (half of a weight tile's rows),
// for the small late layers whose 128-channel tiling leaves half the CUs without a workgroup.
template <bool GN, int NI>
__global__ __launch_bounds__(256, 2) void conv3x3_patch_kernel(PatchArgs p) {
  __shared__ __attribute__((aligned(16))) bf16_t Ws[TILE];
  __shared__ __attribute__((aligned(16))) bf16_t Xp[NPL * XPATCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1;
  const int g = lane >> 4, l16 = lane & 15;
  const int ex = scale_exp(p.x_amax);
  const float unscale = __builtin_ldexpf(1.f, -(ex + scale_exp(p.w_amax)));
  const int per_xcd = gridDim.x >> 3;
  const int tile = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);     // contiguous band of tiles per XCD
  if (tile >= p.ntiles) return;
  const int nblk = NI == 4 ? blockIdx.y : blockIdx.y >> 1, nhalf = NI == 4 ? 0 : blockIdx.y & 1;
  const int tx = tile % p.tiles_x, ty = (tile / p.tiles_x) % p.tiles_y, b = tile / (p.tiles_x * p.tiles_y);
  const int y0 = ty * PT_H, x0 = tx * PT_W;

  // patch element e = tid + 256 i: patch pixel e >> 3, channel quad e & 7; the pixel's address is fixed for the kernel
  const int q = tid & 7;
  const float* ppix[6];
  bool pok[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int prow = (tid >> 3) + 32 * i;
    const int iy = y0 + prow / PP_W - 1, ix = x0 + prow % PP_W - 1;
    pok[i] = prow < PP_ROWS && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && q * 4 < p.Cin;   // (Cin = 4: one quad of the slab)
    ppix[i] = pok[i] ? p.x + (((int64_t)b * p.H + iy) * p.W + ix) * p.Cin + q * 4 : p.x;
  }

  f32x4_t acc[NI][4];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  f32x4_t rx[6];
  // weight tile: NI == 4 all 128 rows of each plane (4 x 16 B per thread); NI == 2 this workgroup's 64 rows of each plane
  // (2 x 16 B per thread, one plane per piece), parked at rows 0..63 of the plane's LDS image
  constexpr int WPIECES = NI == 4 ? 4 : 2;
  constexpr int WSTEP = NI == 4 ? 256 : PLANE / 8;              // 16-byte units between a thread's pieces
  u32x4_t rw[WPIECES];
  const u32x4_t* wbase = reinterpret_cast<const u32x4_t*>(p.w) + (int64_t)nblk * (TILE / 8) + nhalf * 256 + tid;
  auto fetch_w = [&](int slab, int tap) __attribute__((always_inline)) {
    const u32x4_t* wt = wbase + ((int64_t)tap * p.kslabs + slab) * p.nblks * (TILE / 8);
#pragma unroll
    for (int i = 0; i < WPIECES; ++i) rw[i] = wt[i * WSTEP];
  };
  auto stash_w = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < WPIECES; ++i) reinterpret_cast<u32x4_t*>(Ws)[i * WSTEP + tid] = rw[i];
  };
  auto fetch_x = [&](int slab) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 6; ++i) rx[i] = *reinterpret_cast<const f32x4_t*>(pok[i] ? ppix[i] + slab * SBK : p.x);
  };
  auto stash_x = [&](int slab) __attribute__((always_inline)) {
    float mu = 0.f, rstd = 1.f;
    f32x4_t ga = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
    if constexpr (GN) {
      const int c = slab * SBK + q * 4;
      const float2 mr = p.mu_rstd[b * p.G + c / p.cpg];         // cpg >= 4: a quad never straddles groups
      mu = mr.x; rstd = mr.y;
      ga = *reinterpret_cast<const f32x4_t*>(p.gamma + c);
      be = *reinterpret_cast<const f32x4_t*>(p.beta + c);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int prow = (tid >> 3) + 32 * i;
      if (prow >= PP_ROWS) continue;
      f32x4_t v = rx[i];
      if constexpr (GN) v = gn_swish_quad(v, mu, rstd, ga, be, p.swish);
      if (!pok[i]) v = f32x4_t{0.f, 0.f, 0.f, 0.f};             // the conv pads the NORMALISED tensor with zeros
      store_split_quad(Xp, XPATCH, prow, q, v, ex);
    }
  };

  fetch_x(0);
  fetch_w(0, 0);
  stash_x(0);
  stash_w();
  __syncthreads();
  const bf16_t* wl = Ws + swz(wn * (NI * 16) + l16, g);
  for (int slab = 0; slab < p.kslabs; ++slab) {
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const bool last_tap = tap == 8, more = !(last_tap && slab + 1 == p.kslabs);
      if (more) fetch_w(last_tap ? slab + 1 : slab, last_tap ? 0 : tap + 1);
      if (last_tap && more) fetch_x(slab + 1);
      const int dy = tap / 3, dx = tap - dy * 3;
      const bf16_t* xj[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) xj[j] = Xp + swz((wm * 4 + j + dy) * PP_W + l16 + dx, g);
      mma_slab<XPATCH, NI>(wl, xj, acc);
      __syncthreads();
      if (more) stash_w();
      if (last_tap && more) stash_x(slab + 1);
      __syncthreads();
    }
  }

  // epilogue: block (i, j): channels n..n+3 of output pixel (y0 + 4 wm + j, x0 + l16)
  const int ox = x0 + l16;
  QuadStats qs[NI];
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) qs[i] = QuadStats{0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int oy = y0 + wm * 4 + j;
    if (oy >= p.H || ox >= p.W) continue;
    const int64_t m = ((int64_t)b * p.H + oy) * p.W + ox;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = nblk * SBN + nhalf * 64 + wn * (NI * 16) + i * 16 + g * 4;
      if (n >= p.Cout) continue;
      const f32x4_t v = store_out_quad(acc[i][j], unscale, p.bias ? p.bias + n : nullptr, p.res ? p.res + m * p.Cout + n : nullptr,
                                       p.y + m * p.Cout + n, 0);
      qs[i].add(v);
      mx = fmaxf(mx, quad_absmax(v));
    }
  }
  if (p.stats_out) {
    __syncthreads();                                         // the weight tile's LDS is free now
    flush_quad_stats<NI>(qs, mx, reinterpret_cast<double*>(Ws), wn * NI * 4, g, l16, tid, nblk * SBN + nhalf * 64, p.Cout, p.out_cpg,
                         p.stats_out + (int64_t)b * (p.Cout / p.out_cpg) * 2, p.amax_out);
  }
}
