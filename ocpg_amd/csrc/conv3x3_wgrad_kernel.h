// The kernel of csrc/conv3x3_wgrad.hip, included there once per 16-bit storage type with WGRAD_KERNEL (its name: conv3x3_wgrad for bf16,
// conv3x3_wgrad_f16 for fp16) and WGRAD_ELEM (its element trait, Bf16 / Fp16) defined: ONE body, and the bf16 kernel compiles to what
// it was (see conv3x3_mfma_kernel.h).
// S = stride, SEG = output pixels per chunk (64 / 32), XW = input columns per chunk incl. the halo
template <int S, int SEG>
#ifdef WG_ONE_SET
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void WGRAD_KERNEL(
#else
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(1, 1))) void WGRAD_KERNEL(
#endif
    const WGRAD_ELEM::T* __restrict__ gz, const WGRAD_ELEM::T* __restrict__ x, WG g,
                                                    WGRAD_ELEM::T* __restrict__ part) {
  using E = WGRAD_ELEM;
  using T = E::T;
  constexpr int XW = (SEG - 1) * S + 3;
  constexpr int GL = SEG * 8 / NT;                       // 16-byte loads per thread and chunk: gz segment
  constexpr int XL = (3 * XW * 8 + NT - 1) / NT;         // ... and the three input rows
  __shared__ __attribute__((aligned(16))) short Gs[SEG * LROW];
  __shared__ __attribute__((aligned(16))) short Xs[3 * XW * LROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int co0 = blockIdx.x * TM, ci0 = blockIdx.y * TN;
  const long long rows = (long long)g.N * g.Ho;
  const long long r_lo = (long long)blockIdx.z * g.rows_per_split, r_hi = min(rows, r_lo + g.rows_per_split);
  const int nseg = (g.Wo + SEG - 1) / SEG;
  const int nchunks = (int)(r_hi > r_lo ? r_hi - r_lo : 0) * nseg;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // Global loads of chunk c + 1 are issued before chunk c is multiplied (registers), parked after it: one workgroup per SIMD set (the nine
  // accumulator tiles take 144 registers) leaves nothing else to hide a load behind.  Loads are unconditional on clamped addresses and
  // zeroed at park time (a load inside a branch waits for its own data before the next one is issued).
  struct Regs { uint4 rg[GL], rx[XL]; unsigned zg, zx; };   // z bit i: element i is padding / outside the map -> parked as zeros
  Regs RA, RB;                                           // two chunks in flight: one chunk's MFMAs (~1 us) do not cover an HBM round trip
  // the fetch cursor (image, output row, segment) advances without divisions; past the last chunk it stays on valid memory
  const long long r0c = min(r_lo, rows - 1);
  int fn = (int)(r0c / g.Ho), fy = (int)(r0c - (long long)fn * g.Ho), fs = 0;
  auto fetch = [&](Regs& R) __attribute__((always_inline)) {
    uint4 (&rg)[GL] = R.rg; uint4 (&rx)[XL] = R.rx;
    unsigned zg = 0, zx = 0;
    const int xo0 = fs * SEG, npx = min(SEG, g.Wo - xo0);
    const long long grow = ((long long)fn * g.Ho + fy) * g.Wo;
#pragma unroll
    for (int i = 0; i < GL; ++i) {
      const int e = tid + i * NT, k = e >> 3, sg = e & 7;
      const bool ok = k < npx && co0 + sg * 8 + 8 <= g.Cout;
      zg |= ok ? 0u : 1u << i;
      rg[i] = *reinterpret_cast<const uint4*>(gz + (grow + min(xo0 + k, g.Wo - 1)) * g.Cout + min(co0 + sg * 8, g.Cout - 8));
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int e = min(tid + i * NT, 3 * XW * 8 - 1), sg = e & 7, j = (e >> 3) % XW, ky = (e >> 3) / XW;
      const int yi = fy * S + ky - 1, xi = xo0 * S - 1 + j;
      const bool ok = yi >= 0 && yi < g.H && xi >= 0 && xi < g.W && ci0 + sg * 8 + 8 <= g.Cin;
      zx |= ok ? 0u : 1u << i;
      rx[i] = *reinterpret_cast<const uint4*>(x + (((long long)fn * g.H + min(max(yi, 0), g.H - 1)) * g.W + min(max(xi, 0), g.W - 1)) * g.Cin +
                                              min(ci0 + sg * 8, g.Cin - 8));
    }
    R.zg = zg, R.zx = zx;
    // advance (never past the workgroup's last row: the extra fetches after the last chunk re-read it)
    if (fs + 1 < nseg) ++fs;
    else if ((long long)fn * g.Ho + fy + 1 < r_hi) { fs = 0; if (++fy == g.Ho) { fy = 0; ++fn; } }
  };
  auto park = [&](const Regs& R) __attribute__((always_inline)) {
    const uint4 (&rg)[GL] = R.rg; const uint4 (&rx)[XL] = R.rx;
    const unsigned zg = R.zg, zx = R.zx;
#pragma unroll
    for (int i = 0; i < GL; ++i) {
      const int e = tid + i * NT;
      *reinterpret_cast<uint4*>(Gs + (e >> 3) * LROW + (e & 7) * 8) = keep(rg[i], !((zg >> i) & 1u));
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int e = tid + i * NT;
      if (e < 3 * XW * 8) *reinterpret_cast<uint4*>(Xs + (e >> 3) * LROW + (e & 7) * 8) = keep(rx[i], !((zx >> i) & 1u));
    }
  };
  fetch(RA);
#ifndef WG_ONE_SET
  fetch(RB);
#endif
  int ps = 0;                                            // segment of the chunk being parked
  auto chunk = [&](Regs& R) __attribute__((always_inline)) {
    const int npx = min(SEG, g.Wo - ps * SEG), kp = (npx + 15) & ~15;
    if (++ps == nseg) ps = 0;
    __syncthreads();                                     // the previous chunk's fragment reads are done
#ifndef WG_CUT_LOAD
    park(R);
    __syncthreads();
    fetch(R);                                            // two chunks ahead (unconditional)
#endif
#ifndef WG_CUT_COMPUTE
    for (int k0 = 0; k0 < kp; k0 += 16) {
      const bf16x8 a = tr_frag(Gs, k0, 1, wm * 32, lane);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t - ky * 3;
        const bf16x8 b = tr_frag(Xs + ky * XW * LROW, k0 * S + kx, S, wn * 32, lane);
        acc[t] = E::mfma(a, b, acc[t]);
      }
    }
#endif
  };
#ifdef WG_ONE_SET
  for (int c = 0; c < nchunks; ++c) chunk(RA);
#else
  for (int c = 0; c < nchunks; c += 2) {
    chunk(RA);
    if (c + 1 < nchunks) chunk(RB);
  }
#endif
  // ---- partial tile -> part[z][co][tap][ci] (the storage type).  C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int ci = ci0 + wn * 32 + (lane & 31);
  if (ci < g.Cin) {
    T* out = part + (long long)blockIdx.z * g.Cout * 9 * g.Cin;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (co < g.Cout) out[((long long)co * 9 + t) * g.Cin + ci] = E::narrow(acc[t][r]);
      }
  }
}
