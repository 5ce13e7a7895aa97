// The two kernels of csrc/small_linear.hip, included there once per 16-bit storage type with
//   SL_FWD / SL_BWD  the kernels' names (sl_fwd / sl_bwd: bf16, sl_fwd_f16 / sl_bwd_f16: fp16)
//   SL_ELEM          their element trait (Bf16 / Fp16 of that file: MFMA opcode, narrowing, widening)
// defined: ONE body, as csrc/conv3x3_mfma_kernel.h -- the bf16 kernels keep the names, signatures and code they had.
__global__ __launch_bounds__(NT) void SL_FWD(const void* __restrict__ x, int x_f32, const short* __restrict__ w, const short* __restrict__ b,
                                             int R, int Cin, int Cout, int relu, short* __restrict__ y) {
  using E = SL_ELEM;
  __shared__ __attribute__((aligned(16))) short As[T * LROW], Bs[T * LROW];
  const int n0 = blockIdx.x * T, m0 = blockIdx.y * T;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  acc = k_loop<E, false, false>((Cin + T - 1) / T, As, Bs, [&](int k0) { return load_seg<E>(x, x_f32, Cin, m0, k0, R, Cin); },
                                [&](int k0) { return load_seg<E>(w, 0, Cin, n0, k0, Cout, Cin); }, acc);
  store_tile<E>(y, 0, Cout, m0, n0, R, Cout, acc, b, relu);
}

// blocks [0, n_dx): gx tiles (M = R, N = Cin, K = Cout);  blocks [n_dx, ..): gw tiles (M = Cout, N = Cin, K = R) + gb from the n-tile 0 column
__global__ __launch_bounds__(NT) void SL_BWD(const void* __restrict__ gy, int gy_f32, const void* __restrict__ x, int x_f32,
                                             const short* __restrict__ w, const short* __restrict__ ymask, int R, int Cin, int Cout, int n_dx,
                                             int need_gx, void* __restrict__ gx, short* __restrict__ gw, short* __restrict__ gb) {
  using E = SL_ELEM;
  __shared__ __attribute__((aligned(16))) short As[T * LROW], Bs[T * LROW];
  const int ntn = (Cin + T - 1) / T;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  if ((int)blockIdx.x < n_dx) {
    if (!need_gx) return;
    const int m0 = (blockIdx.x / ntn) * T, n0 = (blockIdx.x % ntn) * T;
    // A[m = r][k = co] = gy;  B[n = ci][k = co] = w[co][ci]
    acc = k_loop<E, false, true>((Cout + T - 1) / T, As, Bs, [&](int k0) { return load_seg<E>(gy, gy_f32, Cout, m0, k0, R, Cout, ymask); },
                                 [&](int k0) { return load_seg<E>(w, 0, Cin, k0, n0, Cout, Cin); }, acc);
    store_tile<E>(gx, x_f32, Cin, m0, n0, R, Cin, acc, nullptr);
  } else {
    const int t = blockIdx.x - n_dx;
    const int m0 = (t / ntn) * T, n0 = (t % ntn) * T;                   // m = co, n = ci
    const bool do_bias = gb && (t % ntn) == 0;
    // A[m = co][k = r] = gy[r][co];  B[n = ci][k = r] = x[r][ci]
    acc = k_loop<E, true, true>((R + T - 1) / T, As, Bs, [&](int k0) { return load_seg<E>(gy, gy_f32, Cout, k0, m0, R, Cout, ymask); },
                                [&](int k0) { return load_seg<E>(x, x_f32, Cin, k0, n0, R, Cin); }, acc);
    store_tile<E>(gw, 0, Cin, m0, n0, Cout, Cin, acc, nullptr);
    if (do_bias) {
      // bias gradient = column sum of gy in fp32 from the ORIGINAL values (ATen reduces the fp32 gradient before the cast; summing
      // the 16-bit-rounded staged tile lost precision for heads with many rows -- ADVICE r2).  All 256 threads: 64 columns x 4 row
      // phases, 8 independent loads in flight per thread (a serial loop by 64 threads measured 110 us at 600 rows), LDS reduce.
      __syncthreads();
      float* red = reinterpret_cast<float*>(As);                        // [4][64] partial sums
      const int cq = threadIdx.x & 63, rq = threadIdx.x >> 6;
      const int co = m0 + cq;
      float bsum = 0.f;
      if (co < Cout) {
        for (int r0 = rq; r0 < R; r0 += 32) {
          float g[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int r = r0 + 4 * u;
            const long long i = (long long)min(r, R - 1) * Cout + co;
            float v = gy_f32 ? reinterpret_cast<const float*>(gy)[i] : E::widen(reinterpret_cast<const short*>(gy)[i]);
            if (ymask && !(E::widen(ymask[i]) > 0.f)) v = 0.f;
            g[u] = r < R ? v : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) bsum += g[u];
        }
      }
      red[rq * 64 + cq] = bsum;
      __syncthreads();
      if (threadIdx.x < T && co < Cout) gb[co] = E::f2b(red[cq] + red[64 + cq] + red[128 + cq] + red[192 + cq]);
    }
  }
}
