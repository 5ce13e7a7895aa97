// The ring kernel of csrc/conv3x3_wgrad.hip, included there once per 16-bit storage type with WGRAD_RING_KERNEL (its name) and WGRAD_ELEM
// (its element trait) defined, like conv3x3_wgrad_kernel.h.  Same tile (64 co x 64 ci x nine taps), same split over output rows, same
// part[z][co][9][ci]; maps of ONE segment per output row (Wo <= SEG) only -- the entry point declines the others.  What differs:
//   * input rows live in an LDS ring of R = 3 + S slots [XW][LROW]: a step parks only the S rows the ring does not hold yet.  A workgroup's
//     first row and every image boundary are served by P = 3 - S "phantom" steps in front (the P output rows above: they park their
//     rows -- the padding row as zeros -- and multiply nothing), so the fetch / park stream stays uniform;
//   * Gs is double-buffered and step t + 1 is parked while step t multiplies: one barrier per step;
//   * 8 waves: waves 0-3 own taps 0-4, waves 4-7 taps 5-8 (80 / 64 accumulator registers), each group 2 x 2 over the tile: two waves per SIMD.
// Every accumulator still belongs to one wave and sees the same 16-pixel k steps in the same order (output row ascending, pixels
// ascending, padded to 16 with zeros), so every element of `part` is bit-identical to conv3x3_wgrad's.
// S = stride, SEG = output pixels per step (64 / 32), KS = k steps of 16 pixels a row takes (the multiply loop is unrolled: the reads of
// one k step are issued under the MFMAs of the one before), XW = input columns per step incl. the halo
template <int S, int SEG, int KS>
__global__ __launch_bounds__(NTR) void WGRAD_RING_KERNEL(const WGRAD_ELEM::T* __restrict__ gz, const WGRAD_ELEM::T* __restrict__ x, WG g,
                                                         WGRAD_ELEM::T* __restrict__ part) {
  using E = WGRAD_ELEM;
  using T = E::T;
  constexpr int XW = (SEG - 1) * S + 3;
  constexpr int R = 3 + S, P = 3 - S;                    // ring slots (3 live rows + the incoming ones); phantom steps in front of an image's first row
  constexpr int XL = (S * XW * 8 + NTR - 1) / NTR;       // 16-byte loads per thread and step: the S new input rows (the gz row takes one more)
  constexpr int NST = S == 1 ? 4 : 3;                    // steps of global loads in flight (registers: 12 / 16 a step)
  constexpr int GSZ = SEG * LROW, SLOT = XW * LROW;
  __shared__ __attribute__((aligned(16))) short lds[2 * GSZ + R * SLOT];
  short* const Gs = lds;                                 // [2][SEG][LROW]
  short* const Xs = lds + 2 * GSZ;                       // [R][XW][LROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, wm = wave & 1, wn = (wave >> 1) & 1;      // tap group; place in the group's 2 x 2 over the tile
  const int co0 = blockIdx.x * TM, ci0 = blockIdx.y * TN;
  const long long rows = (long long)g.N * g.Ho;
  const long long r_lo = (long long)blockIdx.z * g.rows_per_split, r_hi = min(rows, r_lo + g.rows_per_split);
  constexpr int kp = KS * 16;                            // Wo <= SEG, one segment per output row, padded to 16: (Wo + 15) / 16 = KS k steps
  const long long r0c = min(r_lo, rows - 1);
  const int n0 = (int)(r0c / g.Ho), y0 = (int)(r0c - (long long)n0 * g.Ho);
  // steps of this workgroup: its rows, plus P phantom steps at its first row and after every image boundary inside its range
  const int nsteps = r_hi > r_lo ? (int)(r_hi - r_lo) + P * (1 + (int)((r_hi - 1) / g.Ho) - n0) : 0;
  f32x16 acc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // Loads are unconditional on clamped addresses and zeroed at park time, as in conv3x3_wgrad; NST steps of them are in flight.
  struct Regs { uint4 rg, rx[XL]; unsigned zr; };        // zr bit r (uniform): new input row r lies outside the map -> parked as zeros
  Regs RA, RB, RC, RD;
  // What a thread's loads and parks do not share with the step is computed once: the element's offset inside its map row (an int: the entry
  // point declines maps whose rows hold 2^31 elements or more), its LDS offset inside a slot, which of the S new rows it belongs to (rsel bit i)
  // and whether its column / channels are padding (zc bit 0: the gz element, bit 1 + i: x element i).  A step adds a uniform row base.
  // Where the elements do not fill the last round of loads (or, the gz row, the workgroup), a thread takes an element a second time: the
  // same bytes to the same LDS address, so that neither a load nor a park stands inside a branch.
  int goff, gl, xoff[XL], xl[XL];
  unsigned zc = 0, rsel = 0;
  {
    const int e = tid & (SEG * 8 - 1), k = e >> 3, sg = e & 7;
    zc |= (k < g.Wo && co0 + sg * 8 + 8 <= g.Cout) ? 0u : 1u;
    goff = min(k, g.Wo - 1) * g.Cout + min(co0 + sg * 8, g.Cout - 8);
    gl = k * LROW + sg * 8;
  }
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    int e = tid + i * NTR;
    if (e >= S * XW * 8) e -= NTR;
    const int sg = e & 7, j = (e >> 3) % XW, r = (e >> 3) / XW, xi = j - 1;
    zc |= (xi >= 0 && xi < g.W && ci0 + sg * 8 + 8 <= g.Cin) ? 0u : 2u << i;
    rsel |= r ? 1u << i : 0u;
    xoff[i] = min(max(xi, 0), g.W - 1) * g.Cin + min(ci0 + sg * 8, g.Cin - 8);
    xl[i] = j * LROW + sg * 8;
  }
  // the fetch cursor (image, virtual output row) advances without divisions; past the last step it stays on valid memory
  int fn = n0, fy = y0 - P;
  auto fetch = [&](Regs& R_) __attribute__((always_inline)) {
    R_.rg = *reinterpret_cast<const uint4*>(gz + ((long long)fn * g.Ho + max(fy, 0)) * g.Wo * g.Cout + goff);
    const int y_0 = fy * S + 2 - S, y_1 = y_0 + S - 1;   // the S newest input rows of output row fy
    const int c_0 = min(max(y_0, 0), g.H - 1), c_1 = min(max(y_1, 0), g.H - 1);
    const T* row0 = x + ((long long)fn * g.H + c_0) * g.W * g.Cin;
    const int drow = (c_1 - c_0) * g.W * g.Cin;          // 0 or one map row
#pragma unroll
    for (int i = 0; i < XL; ++i) R_.rx[i] = *reinterpret_cast<const uint4*>(row0 + (xoff[i] + (((rsel >> i) & 1u) ? drow : 0)));
    R_.zr = ((y_0 < 0 || y_0 >= g.H) ? 1u : 0u) | ((y_1 < 0 || y_1 >= g.H) ? 2u : 0u);
    // advance (never past the workgroup's last row: the extra fetches after the last step re-read it)
    if (fy < 0 || (long long)fn * g.Ho + fy + 1 < r_hi) {
      if (++fy == g.Ho) { fy = -P; ++fn; }
    }
  };
  int pb = 0, ps = 0;                                    // park cursor: Gs buffer, first ring slot of the step being parked
  auto park = [&](const Regs& R_) __attribute__((always_inline)) {
    *reinterpret_cast<uint4*>(Gs + pb * GSZ + gl) = keep(R_.rg, !(zc & 1u));
    const int s_0 = ps * SLOT, s_1 = (ps + 1 >= R ? ps + 1 - R : ps + 1) * SLOT;
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const bool second = S == 2 && ((rsel >> i) & 1u);
      const bool zero = ((zc >> (1 + i)) & 1u) || ((R_.zr >> (second ? 1 : 0)) & 1u);
      *reinterpret_cast<uint4*>(Xs + (second ? s_1 : s_0) + xl[i]) = keep(R_.rx[i], !zero);
    }
    pb ^= 1;
    ps += S;
    if (ps >= R) ps -= R;
  };
  int cb = 0, cs = 0, cy = y0, ph = P;                   // compute cursor: Gs buffer, first ring slot the step parked, output row, phantom steps in front of it
  auto mult = [&](auto first, auto count) __attribute__((always_inline)) {
    constexpr int T0 = decltype(first)::value, NTAP = decltype(count)::value;
    int row[3];                                          // ring slot of input row ky: the step's own S rows are the newest
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      int s = cs + ky + S - 3;
      if (s < 0) s += R;
      if (s >= R) s -= R;
      row[ky] = s * SLOT;
    }
#pragma unroll
    for (int k0 = 0; k0 < kp; k0 += 16) {
      const bf16x8 a = tr_frag(Gs + cb * GSZ, k0, 1, wm * 32, lane);
#pragma unroll
      for (int t = 0; t < NTAP; ++t) {
        const int ky = (T0 + t) / 3, kx = (T0 + t) - ky * 3;
        const bf16x8 b = tr_frag(Xs + row[ky], k0 * S + kx, S, wn * 32, lane);
        acc[t] = E::mfma(a, b, acc[t]);
      }
    }
  };
  // one step: park step t + 1 (the free Gs buffer, the free ring slots), refill its registers NST steps ahead, multiply step t
  auto step = [&](Regs& R_) __attribute__((always_inline)) {
#ifndef WG_CUT_LOAD
    park(R_);
    fetch(R_);
#endif
#ifndef WG_CUT_COMPUTE
    if (ph == 0) {
      if (grp == 0) mult(IC<0>{}, IC<5>{});
      else mult(IC<5>{}, IC<4>{});
    }
#endif
    cb ^= 1;
    cs += S;
    if (cs >= R) cs -= R;
    if (ph > 0) --ph;
    else if (++cy == g.Ho) { cy = 0; ph = P; }
    __syncthreads();                                     // step t + 1 is parked; step t's fragment reads are done
  };
  // waves 4-7 are dispatched later and would lose every issue arbitration to their SIMD partners by age: one static priority for the
  // whole kernel evens that out (measured: 31.7 -> 30.6 us at layer3, 42.2 -> 39.4 us at layer4, cold operands)
  if (grp) __builtin_amdgcn_s_setprio(1);
  fetch(RA); fetch(RB);
  if constexpr (NST >= 3) fetch(RC);
  if constexpr (NST == 4) fetch(RD);
#ifndef WG_CUT_LOAD
  park(RA);
  fetch(RA);
#endif
  __syncthreads();
  // (left by `break`, not one `if` per step: a step that may have been skipped makes the compiler count its loads as not issued, and
  // the next park then waits for younger loads as well)
  if (nsteps > 0)
    for (int c = 0;;) {
      step(RB);
      if (++c >= nsteps) break;
      if constexpr (NST >= 3) {
        step(RC);
        if (++c >= nsteps) break;
      }
      if constexpr (NST == 4) {
        step(RD);
        if (++c >= nsteps) break;
      }
      step(RA);
      if (++c >= nsteps) break;
    }
  // ---- partial tile -> part[z][co][tap][ci] (the storage type), as conv3x3_wgrad writes it
  const int ci = ci0 + wn * 32 + (lane & 31);
  if (ci < g.Cin) {
    T* out = part + (long long)blockIdx.z * g.Cout * 9 * g.Cin;
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int tap = grp * 5 + t;
        if (tap < 9 && co < g.Cout) out[((long long)co * 9 + tap) * g.Cin + ci] = E::narrow(acc[t][r]);
      }
  }
}
