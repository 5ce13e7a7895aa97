// The LFM block's two Fourier transforms with a CHIRP-Z (Bluestein) line transform on one or both axes: a line of ANY length 65 <= L <= 128
// -- the primes 67..127 are what it is for: from 83 on the direct O(p^2) stage of csrc/lfm_dft_any.hip loses to the library -- becomes a cyclic
// convolution of fixed length M = 256, which two butterfly FFTs serve:
//     X_k = c_k * IFFT_M(FFT_M(a) * B)_k,   a_n = x_n c_n (n < L, zero up to M),   c_n = exp(-i pi n^2 / L),   B = FFT_M(wrapped conj(c))
// (n k = (n^2 + k^2 - (k - n)^2) / 2).  The inverse direction uses conj(c) and the matching B; nothing depends on L being prime.
// The same four passes with the same contracts as lfm_dft_any.hip (rows_fwd, cols_fwd, cols_inv, rows_inv; channels-last maps, a lane owns
// one channel of a line, half spectrum along w, fp32 arithmetic, no atomics, no memset, two launches per direction, every size by value).
// An axis that is NOT a chirp axis runs lfm_dft_any.hip's own kernel for that pass (lfm_dft_any_kernel.h): the passes meet in tmp, which
// holds the half spectrum in natural order whichever kernel wrote it.
//
// The M-point transforms: M = 16 x 16, two radix-16 stages, each 16-point DFT held in 32 registers and built from two levels of radix-4
// butterflies (the +-1 / +-i factors cost no multiply; nine constant twiddles between the levels).  Forward = decimation in frequency
// (natural in, digit-reversed out), inverse = decimation in time (digit-reversed in, natural out), B stored digit-reversed (and divided by
// M): no reordering pass, and the LAST forward stage, the product with B and the FIRST inverse stage work on the same 16 slots, so they
// stay in registers.  With slot s of the LDS tile [256][CHW] float2:
//   first  group r  (16 of them): a[16 j + r], j < 8 (L <= 128: the upper eight inputs are zero) straight from GLOBAL memory through the
//                   pass's prologue -> 16-point DFT over j -> * W_256^(r k1) -> slot 16 k1 + r
//   middle group k1: slots 16 k1 + r -> DFT over r: A[k1 + 16 k2] -> * B -> inverse DFT over k2 -> * W_256^-(m2 k1) -> slot 16 k1 + m2
//   last   group m2: slots 16 k1 + m2 -> inverse DFT over k1: y[m2 + 16 m1], only m1 < 8 (5 for a half spectrum) are formed
//                   -> * c -> the pass's epilogue straight to GLOBAL memory
// Two barriers and two LDS round trips per line.  A workgroup has 256 threads and 32 channels: the tile is 64 KB (two workgroups per CU),
// lanes 0..31 and 32..63 of a wave take two DIFFERENT groups of the same 32 channels, eight groups at a time, two rounds per stage.  The
// chirp, B and W_256 factors depend on the group only: both halves' values are wave-uniform (scalar) loads and a select picks one.
#include "lfm_dft_any_kernel.h"

namespace {

constexpr int CZ_MINL = 65, CZ_MAXL = 128;               // M = 256 >= 2 L - 1
constexpr int CZ_C = 0, CZ_BF = 128, CZ_BI = 384, CZ_W = 640;      // the table (include/ocpg_hip.h), float2 offsets
// channels per workgroup: 32 (64 KB of LDS, two workgroups per CU; measured faster).  A diagnostic build with -DOCPG_CZT_CHW=64
// runs the other layout the kernels are written for: a wave takes ONE group of 64 channels, 128 KB, one workgroup per CU.
#ifndef OCPG_CZT_CHW
#define OCPG_CZT_CHW 32
#endif
constexpr int CZ_CHW = OCPG_CZT_CHW, CZ_NT = 256;
static_assert(CZ_CHW == 32 || CZ_CHW == 64, "a wave holds one or two groups");

__device__ __forceinline__ float2 ad(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 sb(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// * W_4 = -i (forward), +i (inverse)
template <bool INV> __device__ __forceinline__ float2 rot(float2 a) { return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }

template <bool INV> __device__ __forceinline__ void fft4(float2& a, float2& b, float2& c, float2& d) {
  const float2 t0 = ad(a, c), t1 = sb(a, c), t2 = ad(b, d), t3 = rot<INV>(sb(b, d));
  a = ad(t0, t2), b = ad(t1, t3), c = sb(t0, t2), d = sb(t1, t3);
}

// * W_16^M (conjugated when INV), M one of the products j0 * k0 below
template <int M, bool INV> __device__ __forceinline__ float2 tw16(float2 v) {
  constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, HF = 0.70710678118654752f;
  static_assert(M == 1 || M == 2 || M == 3 || M == 4 || M == 6 || M == 9, "j0 * k0");
  if constexpr (M == 4) {
    return rot<INV>(v);
  } else {
    constexpr float wr = M == 1 ? C1 : M == 2 ? HF : M == 3 ? S1 : M == 6 ? -HF : -C1;      // cos(pi M / 8)
    constexpr float ws = M == 1 ? S1 : M == 2 ? HF : M == 3 ? C1 : M == 6 ? HF : -S1;       // sin(pi M / 8)
    constexpr float wy = INV ? ws : -ws;
    return make_float2(v.x * wr - v.y * wy, v.x * wy + v.y * wr);
  }
}

// where output k of fft16 sits in its register array
__device__ __forceinline__ constexpr int at16(int k) { return 4 * (k & 3) + (k >> 2); }

// the 16-point DFT of r[0..16) in place, output k in r[at16(k)].  j = 4 j1 + j0, k = k0 + 4 k1: radix 4 over j1 for every j0, the twiddle
// W_16^(j0 k0), radix 4 over j0 for every k0.  HALF_IN: r[8..16) are zero (and are not read).
template <bool INV, bool HALF_IN> __device__ __forceinline__ void fft16(float2 (&r)[16]) {
#pragma unroll
  for (int j0 = 0; j0 < 4; ++j0) {
    if (HALF_IN) {
      const float2 a = r[j0], b = r[4 + j0], rb = rot<INV>(b);
      r[j0] = ad(a, b), r[4 + j0] = ad(a, rb), r[8 + j0] = sb(a, b), r[12 + j0] = sb(a, rb);
    } else {
      fft4<INV>(r[j0], r[4 + j0], r[8 + j0], r[12 + j0]);
    }
  }
  // r[4 k0 + j0] *= W_16^(j0 k0)
  r[5] = tw16<1, INV>(r[5]), r[6] = tw16<2, INV>(r[6]), r[7] = tw16<3, INV>(r[7]);
  r[9] = tw16<2, INV>(r[9]), r[10] = tw16<4, INV>(r[10]), r[11] = tw16<6, INV>(r[11]);
  r[13] = tw16<3, INV>(r[13]), r[14] = tw16<6, INV>(r[14]), r[15] = tw16<9, INV>(r[15]);
#pragma unroll
  for (int k0 = 0; k0 < 4; ++k0) fft4<INV>(r[4 * k0], r[4 * k0 + 1], r[4 * k0 + 2], r[4 * k0 + 3]);
}

// who a thread is in a stage: the two halves of a wave take the groups ga and gb of a round, channel ch of the workgroup's CHW
template <int CHW> struct Who {
  static constexpr int G = 64 / CHW, NG = (CZ_NT / 64) * G;
  int wave, ch;
  bool hi;
  __device__ __forceinline__ Who(int lane, int wave_) : wave(wave_), ch(lane % CHW), hi(G == 2 && lane >= CHW) {}
  // entry i0 (lower half's group) or i1 (upper half's) of a table: both indices are wave-uniform
  __device__ __forceinline__ float2 pick(const float2* __restrict__ t, int i0, int i1) const {
    if (G == 1) return t[i0];
    const float2 a = t[i0], b = t[i1];
    return hi ? b : a;
  }
};

// ---- first stage.  ld(n): element n of the line (zero for n >= L and for a channel past C)
template <int CHW, bool INV, bool REAL_IN, typename LD>
__device__ __forceinline__ void czt_first(float2* __restrict__ tile, const float2* __restrict__ cz, const Who<CHW> t, LD ld) {
  constexpr int G = Who<CHW>::G, NG = Who<CHW>::NG;
  for (int it = 0; it < 16 / NG; ++it) {
    const int ga = it * NG + t.wave * G, gb = ga + G - 1, r = t.hi ? gb : ga;
    float2 x[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = ld(16 * j + r);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float2 c = t.pick(cz + CZ_C, 16 * j + ga, 16 * j + gb);
      if (INV) c.y = -c.y;
      x[j] = REAL_IN ? make_float2(x[j].x * c.x, x[j].x * c.y) : cmul(x[j], c);
    }
    fft16<false, true>(x);
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) {
      float2 v = x[at16(k1)];
      if (k1 > 0) v = cmul(v, t.pick(cz + CZ_W, ga * k1, gb * k1));
      tile[(16 * k1 + r) * CHW + t.ch] = v;
    }
  }
}

// ---- last forward stage, * B, first inverse stage: in place on the 16 slots of a group
template <int CHW, bool INV>
__device__ __forceinline__ void czt_mid(float2* __restrict__ tile, const float2* __restrict__ cz, const Who<CHW> t) {
  constexpr int G = Who<CHW>::G, NG = Who<CHW>::NG;
  const float2* __restrict__ B = cz + (INV ? CZ_BI : CZ_BF);
  for (int it = 0; it < 16 / NG; ++it) {
    const int ga = it * NG + t.wave * G, gb = ga + G - 1, k1 = t.hi ? gb : ga;
    float2 x[16], y[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = tile[(16 * k1 + r) * CHW + t.ch];
    fft16<false, false>(x);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) y[k2] = cmul(x[at16(k2)], t.pick(B, 16 * ga + k2, 16 * gb + k2));
    fft16<true, false>(y);
#pragma unroll
    for (int m2 = 0; m2 < 16; ++m2) {
      float2 v = y[at16(m2)];
      if (m2 > 0) {
        float2 w = t.pick(cz + CZ_W, ga * m2, gb * m2);
        w.y = -w.y;
        v = cmul(v, w);
      }
      tile[(16 * k1 + m2) * CHW + t.ch] = v;
    }
  }
}

// ---- last inverse stage.  st(k, X_k) for every k < nout the group holds; NOUT: the m1 that are formed (k = m2 + 16 m1 < 16 NOUT)
template <int CHW, bool INV, int NOUT, typename ST>
__device__ __forceinline__ void czt_last(const float2* __restrict__ tile, const float2* __restrict__ cz, const Who<CHW> t, int nout, ST st) {
  constexpr int G = Who<CHW>::G, NG = Who<CHW>::NG;
  for (int it = 0; it < 16 / NG; ++it) {
    const int ga = it * NG + t.wave * G, gb = ga + G - 1, m2 = t.hi ? gb : ga;
    float2 x[16];
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) x[k1] = tile[(16 * k1 + m2) * CHW + t.ch];
    fft16<true, false>(x);
#pragma unroll
    for (int m1 = 0; m1 < NOUT; ++m1) {
      const int k = m2 + 16 * m1;
      float2 c = t.pick(cz + CZ_C, ga + 16 * m1, gb + 16 * m1);
      if (INV) c.y = -c.y;
      if (k < nout) st(k, cmul(x[at16(m1)], c));
    }
  }
}

// ---- along w, real -> half spectrum.  grid (N*H, ceil(C / CHW)), 256 threads, 256 * CHW float2 of LDS (all four kernels)
template <int CHW>
__global__ __launch_bounds__(CZ_NT) void rows_fwd_czt(const float* __restrict__ x, int W, int C, const float2* __restrict__ cz, float2* __restrict__ T) {
  extern __shared__ float2 tile[];
  const Who<CHW> t(threadIdx.x & 63, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const long long line = blockIdx.x;
  const int c = blockIdx.y * CHW + t.ch;
  const bool ok = c < C;
  const int Wh = W / 2 + 1;
  czt_first<CHW, false, true>(tile, cz, t, [&](int n) { return make_float2((ok && n < W) ? x[(line * W + n) * C + c] : 0.f, 0.f); });
  __syncthreads();
  czt_mid<CHW, false>(tile, cz, t);
  __syncthreads();
  czt_last<CHW, false, 5>(tile, cz, t, Wh, [&](int v, float2 s) {
    if (ok) T[(line * Wh + v) * C + c] = s;
  });
}

// ---- along h, half spectrum -> gated [Re || Im] pair, both mirror halves.  grid (N * (W/2+1), ceil(C / CHW))
template <int CHW, typename P>
__global__ __launch_bounds__(CZ_NT) void cols_fwd_czt(const float2* __restrict__ T, const float* __restrict__ coef, const float* __restrict__ high, int H, int W,
                                                      int C, const float2* __restrict__ cz, float norm, P* __restrict__ pair) {
  extern __shared__ float2 tile[];
  const Who<CHW> t(threadIdx.x & 63, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const int Wh = W / 2 + 1;
  const int n = blockIdx.x / Wh, v = blockIdx.x - n * Wh;
  const int c = blockIdx.y * CHW + t.ch;
  const bool ok = c < C;
  czt_first<CHW, false, false>(tile, cz, t, [&](int y) {
    return (ok && y < H) ? T[(((long long)n * H + y) * Wh + v) * C + c] : make_float2(0.f, 0.f);
  });
  __syncthreads();
  czt_mid<CHW, false>(tile, cz, t);
  __syncthreads();
  const float cf = coef ? coef[n] : 0.f;
  const int vm = W - v;                                   // the mirror column (v = 0 and v = W / 2 mirror onto themselves)
  const bool mirror = v > 0 && vm > v;
  czt_last<CHW, false, 8>(tile, cz, t, H, [&](int u, float2 sv) {
    if (!ok) return;
    const float g = norm * (coef ? 1.f - cf * high[u * W + v] : 1.f);
    P* d = pair + (((long long)n * H + u) * W + v) * 2 * C + c;
    stf(d, sv.x * g);
    stf(d + C, sv.y * g);
    if (mirror) {                                         // S[(H - u) % H][W - v] = conj(S[u][v])
      const int um = u ? H - u : 0;
      const float gm = norm * (coef ? 1.f - cf * high[um * W + vm] : 1.f);
      P* dm = pair + (((long long)n * H + um) * W + vm) * 2 * C + c;
      stf(dm, sv.x * gm);
      stf(dm + C, -sv.y * gm);
    }
  });
}

// ---- pair (* gate) -> Hermitian part -> inverse along h.  grid (N * (W/2+1), ceil(C / CHW)); part [N][(W/2+1) * gridDim.y]
template <int CHW, typename P>
__global__ __launch_bounds__(CZ_NT) void cols_inv_czt(const P* __restrict__ pair, const float* __restrict__ coef, const float* __restrict__ high,
                                                      const P* __restrict__ zs, float* __restrict__ part, int H, int W, int C, const float2* __restrict__ cz,
                                                      float2* __restrict__ T) {
  extern __shared__ float2 tile[];
  const Who<CHW> t(threadIdx.x & 63, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const int Wh = W / 2 + 1;
  const int n = blockIdx.x / Wh, v = blockIdx.x - n * Wh;
  const int c = blockIdx.y * CHW + t.ch;
  const bool ok = c < C;
  const float cf = coef ? coef[n] : 0.f;
  const int vm = v ? W - v : 0;
  float dsum = 0.f;
  czt_first<CHW, true, false>(tile, cz, t, [&](int u) {
    if (!ok || u >= H) return make_float2(0.f, 0.f);
    const int um = u ? H - u : 0;
    const long long ia = (((long long)n * H + u) * W + v) * 2 * C + c, ib = (((long long)n * H + um) * W + vm) * 2 * C + c;
    const float ar = ldf(pair + ia), ai = ldf(pair + ia + C), br = ldf(pair + ib), bi = ldf(pair + ib + C);
    const float ha = coef ? high[u * W + v] : 0.f, hb = coef ? high[um * W + vm] : 0.f;
    const float ga = 1.f - cf * ha, gb = 1.f - cf * hb;
    // d/dcoef of S * (1 - coef * high): -high * (g_re S_re + g_im S_im), with S = z / gate from the saved gated spectrum (a gate
    // of exactly 0 has lost S: that single term is dropped, as in lfm_dft.hip)
    if (part) {
      if (ga != 0.f) dsum -= ha * (ar * ldf(zs + ia) + ai * ldf(zs + ia + C)) / ga;
      if (vm != v && gb != 0.f) dsum -= hb * (br * ldf(zs + ib) + bi * ldf(zs + ib + C)) / gb;
    }
    return make_float2(0.5f * (ar * ga + br * gb), 0.5f * (ai * ga - bi * gb));
  });
  __syncthreads();
  czt_mid<CHW, true>(tile, cz, t);
  __syncthreads();
  czt_last<CHW, true, 8>(tile, cz, t, H, [&](int y, float2 s) {
    if (ok) T[(((long long)n * H + y) * Wh + v) * C + c] = s;
  });
  if (part) {
    float* red = (float*)tile;                            // (the tile is free once every wave has read its last stage)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dsum += __shfl_down(dsum, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[t.wave] = dsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int i = 0; i < CZ_NT / 64; ++i) s += red[i];
      part[((long long)n * Wh + v) * gridDim.y + blockIdx.y] = s;
    }
  }
}

// ---- half spectrum -> real line (+ residual).  grid (N*H, ceil(C / CHW))
template <int CHW>
__global__ __launch_bounds__(CZ_NT) void rows_inv_czt(const float2* __restrict__ T, int W, int C, const float2* __restrict__ cz, float norm,
                                                      const float* __restrict__ residual, float* __restrict__ out) {
  extern __shared__ float2 tile[];
  const Who<CHW> t(threadIdx.x & 63, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const long long line = blockIdx.x;
  const int c = blockIdx.y * CHW + t.ch;
  const bool ok = c < C;
  const int Wh = W / 2 + 1;
  czt_first<CHW, true, false>(tile, cz, t, [&](int v) {
    if (!ok || v >= W) return make_float2(0.f, 0.f);
    const float2 q = T[(line * Wh + (v < Wh ? v : W - v)) * C + c];
    return make_float2(q.x, v < Wh ? q.y : -q.y);
  });
  __syncthreads();
  czt_mid<CHW, true>(tile, cz, t);
  __syncthreads();
  czt_last<CHW, true, 8>(tile, cz, t, W, [&](int j, float2 s) {
    if (!ok) return;
    const long long o = (line * W + j) * C + c;
    out[o] = norm * s.x + (residual ? residual[o] : 0.f);
  });
}

constexpr size_t CZ_LDS = (size_t)256 * CZ_CHW * sizeof(float2);

// above 64 KB a kernel has to be told (the 64-channel diagnostic build only)
template <typename K> inline void big_lds(K kernel) {
  if (CZ_LDS > 65536) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CZ_LDS);
}

inline bool cz_axis_ok(int L, int r1, int r2, int r3) { return L >= CZ_MINL && L <= CZ_MAXL && r1 == 1 && r2 == 1 && r3 == L; }

template <typename P>
void launch_cols_fwd_czt(const void* tmp, const float* coef, const float* high, int N, int H, int W, int C, const void* cz, float norm, void* pair,
                         hipStream_t st) {
  const dim3 g((unsigned)(N * (W / 2 + 1)), (C + CZ_CHW - 1) / CZ_CHW);
  big_lds(cols_fwd_czt<CZ_CHW, P>);
  cols_fwd_czt<CZ_CHW, P><<<g, CZ_NT, CZ_LDS, st>>>((const float2*)tmp, coef, high, H, W, C, (const float2*)cz, norm, (P*)pair);
}

template <typename P>
void launch_cols_inv_czt(const void* pair, const float* coef, const float* high, const void* zs, float* part, int N, int H, int W, int C, const void* cz,
                         void* tmp, hipStream_t st) {
  const dim3 g((unsigned)(N * (W / 2 + 1)), (C + CZ_CHW - 1) / CZ_CHW);
  big_lds(cols_inv_czt<CZ_CHW, P>);
  cols_inv_czt<CZ_CHW, P><<<g, CZ_NT, CZ_LDS, st>>>((const P*)pair, coef, high, (const P*)zs, part, H, W, C, (const float2*)cz, (float2*)tmp);
}

}  // namespace

extern "C" {

int ocpg_lfm_spectrum_fwd_czt(const float* x, const float* coef, const float* high, int N, int H, int W, int C, const void* tw_h, const void* tw_w,
                              float norm, void* tmp, void* pair, int pair_dt, int h1, int h2, int h3, int w1, int w2, int w3, const void* cz_h,
                              const void* cz_w, void* stream) {
  if (N < 0 || H < 1 || W < 1 || C < 1) return -1003;
  if (N == 0) return 0;
  Plan ph{0, 0, {1, 1, 1}, {0, 0, 0}, 0}, pw = ph;
  if (cz_h ? !cz_axis_ok(H, h1, h2, h3) : !(ph = plan_of(H, h1, h2, h3)).L) return -2000;
  if (cz_w ? !cz_axis_ok(W, w1, w2, w3) : !(pw = plan_of(W, w1, w2, w3)).L) return -2000;
  if (!x) return -1001;
  if (!tw_h || !tw_w) return -1005;
  if (!tmp) return -1011;
  if (!pair) return -1012;
  if ((coef == nullptr) != (high == nullptr)) return -1002;
  if (pair_dt < 0 || pair_dt > 2) return -1013;
  hipStream_t st = (hipStream_t)stream;
  const int Wh = W / 2 + 1;
  if ((long long)N * H > 2147483647LL || (long long)N * Wh > 2147483647LL) return -1003;
  if (cz_w) big_lds(rows_fwd_czt<CZ_CHW>);
  if (cz_w)
    rows_fwd_czt<CZ_CHW><<<dim3((unsigned)(N * H), (C + CZ_CHW - 1) / CZ_CHW), CZ_NT, CZ_LDS, st>>>(x, W, C, (const float2*)cz_w, (float2*)tmp);
  else if (chw_of(W) == 64)
    rows_fwd_any<64><<<dim3((unsigned)(N * H), (C + 63) / 64), 256, (size_t)W * 64 * sizeof(float2), st>>>(x, W, C, pw, (const float2*)tw_w, (float2*)tmp);
  else
    rows_fwd_any<32><<<dim3((unsigned)(N * H), (C + 31) / 32), 512, (size_t)W * 32 * sizeof(float2), st>>>(x, W, C, pw, (const float2*)tw_w, (float2*)tmp);
  if (cz_h) {
    if (pair_dt == 0) launch_cols_fwd_czt<float>(tmp, coef, high, N, H, W, C, cz_h, norm, pair, st);
    else if (pair_dt == 1) launch_cols_fwd_czt<__hip_bfloat16>(tmp, coef, high, N, H, W, C, cz_h, norm, pair, st);
    else launch_cols_fwd_czt<__half>(tmp, coef, high, N, H, W, C, cz_h, norm, pair, st);
  } else if (chw_of(H) == 64) {
    if (pair_dt == 0) launch_cols_fwd<64, float>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else if (pair_dt == 1) launch_cols_fwd<64, __hip_bfloat16>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else launch_cols_fwd<64, __half>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
  } else {
    if (pair_dt == 0) launch_cols_fwd<32, float>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else if (pair_dt == 1) launch_cols_fwd<32, __hip_bfloat16>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else launch_cols_fwd<32, __half>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
  }
  return status();
}

int ocpg_lfm_spectrum_inv_czt(const void* pair, int pair_dt, const float* coef, const float* high, const void* z_saved, float* coef_part, int N, int H,
                              int W, int C, const void* tw_h, const void* tw_w, float norm, void* tmp, const float* residual, float* out, int h1, int h2,
                              int h3, int w1, int w2, int w3, const void* cz_h, const void* cz_w, void* stream) {
  if (N < 0 || H < 1 || W < 1 || C < 1) return -1007;
  if (N == 0) return 0;
  Plan ph{0, 0, {1, 1, 1}, {0, 0, 0}, 0}, pw = ph;
  if (cz_h ? !cz_axis_ok(H, h1, h2, h3) : !(ph = plan_of(H, h1, h2, h3)).L) return -2000;
  if (cz_w ? !cz_axis_ok(W, w1, w2, w3) : !(pw = plan_of(W, w1, w2, w3)).L) return -2000;
  if (!pair) return -1001;
  if (!tw_h || !tw_w) return -1011;
  if (!tmp) return -1014;
  if (!out) return -1016;
  if ((coef == nullptr) != (high == nullptr)) return -1003;
  if (coef_part && (!coef || !z_saved)) return -1005;
  if (pair_dt < 0 || pair_dt > 2) return -1002;
  hipStream_t st = (hipStream_t)stream;
  const int Wh = W / 2 + 1;
  if ((long long)N * H > 2147483647LL || (long long)N * Wh > 2147483647LL) return -1007;
  if (cz_h) {
    if (pair_dt == 0) launch_cols_inv_czt<float>(pair, coef, high, z_saved, coef_part, N, H, W, C, cz_h, tmp, st);
    else if (pair_dt == 1) launch_cols_inv_czt<__hip_bfloat16>(pair, coef, high, z_saved, coef_part, N, H, W, C, cz_h, tmp, st);
    else launch_cols_inv_czt<__half>(pair, coef, high, z_saved, coef_part, N, H, W, C, cz_h, tmp, st);
  } else if (chw_of(H) == 64) {
    if (pair_dt == 0) launch_cols_inv<64, float>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else if (pair_dt == 1) launch_cols_inv<64, __hip_bfloat16>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else launch_cols_inv<64, __half>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
  } else {
    if (pair_dt == 0) launch_cols_inv<32, float>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else if (pair_dt == 1) launch_cols_inv<32, __hip_bfloat16>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else launch_cols_inv<32, __half>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
  }
  if (cz_w) big_lds(rows_inv_czt<CZ_CHW>);
  if (cz_w)
    rows_inv_czt<CZ_CHW><<<dim3((unsigned)(N * H), (C + CZ_CHW - 1) / CZ_CHW), CZ_NT, CZ_LDS, st>>>((const float2*)tmp, W, C, (const float2*)cz_w, norm, residual,
                                                                                                out);
  else if (chw_of(W) == 64)
    rows_inv_any<64><<<dim3((unsigned)(N * H), (C + 63) / 64), 256, (size_t)W * 64 * sizeof(float2), st>>>((const float2*)tmp, W, C, pw, (const float2*)tw_w, norm,
                                                                                                        residual, out);
  else
    rows_inv_any<32><<<dim3((unsigned)(N * H), (C + 31) / 32), 512, (size_t)W * 32 * sizeof(float2), st>>>((const float2*)tmp, W, C, pw, (const float2*)tw_w, norm,
                                                                                                        residual, out);
  return status();
}

}  // extern "C"
