// The device code of csrc/lfm_dft_any.hip (its head describes the passes, the plan and the stages), shared with csrc/lfm_dft_czt.hip: there an
// axis that is not a chirp axis runs the same kernels.  Everything sits in an unnamed namespace: each file that includes this header
// compiles its own copies.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int MAXR = 16, MAXL = 256, MAXP = 251;
constexpr int U = 8;                    // global loads of a line in flight per thread
constexpr int NU = 4, KB = 8;           // direct stage: units of KB outputs a wave holds in registers

// s[0..ns): the stages that are not 1, in order; off[i]: where the s[i] x s[i] DFT matrix starts in the table (stages <= 16);
// slot: where the table of output slots (int[L]) starts, both in float2 units
struct Plan { int L, ns, s[3], off[3], slot; };

inline bool is_prime(int v) {
  if (v < 2) return false;
  for (int d = 2; d * d <= v; ++d)
    if (v % d == 0) return false;
  return true;
}

// the plan of one axis, or L = 0: refused (product, range, more than one stage above 16, a stage above 16 that is not a prime <= 251)
inline Plan plan_of(int L, int r1, int r2, int r3) {
  Plan p{0, 0, {1, 1, 1}, {0, 0, 0}, 0};
  if (L < 1 || L > MAXL || r1 < 1 || r2 < 1 || r3 < 1) return p;
  if ((long long)r1 * r2 * r3 != L) return p;
  const int r[3] = {r1, r2, r3};
  int big = 0, off = L;
  for (int i = 0; i < 3; ++i) {
    if (r[i] == 1) continue;
    if (r[i] > MAXR) {
      if (r[i] > MAXP || !is_prime(r[i]) || ++big > 1) return p;
    } else {
      p.off[p.ns] = off;
      off += r[i] * r[i];
    }
    p.s[p.ns++] = r[i];
  }
  p.slot = off;
  p.L = L;
  return p;
}

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return (float)*p; }
template <> __device__ __forceinline__ float ldf<__hip_bfloat16>(const __hip_bfloat16* p) { return __bfloat162float(*p); }
template <> __device__ __forceinline__ float ldf<__half>(const __half* p) { return __half2float(*p); }
template <typename T> __device__ __forceinline__ void stf(T* p, float v) { *p = (T)v; }
template <> __device__ __forceinline__ void stf<__hip_bfloat16>(__hip_bfloat16* p, float v) { *p = __float2bfloat16(v); }
template <> __device__ __forceinline__ void stf<__half>(__half* p, float v) { *p = __float2half(v); }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// what every stage is told.  kd: the last stage of three finds the spectrum index of its batch kp = k0 s1 + k1 as k0 + s0 k1 with
// kd = s1 (P / kd = s0); otherwise kd = 1 and the index is kp itself
struct Stage { int L, P, Q, kd, kmax; bool last; };

__device__ __forceinline__ int kbase(const Stage& g, int kp) { return g.last ? kp / g.kd + (kp % g.kd) * (g.P / g.kd) : 0; }

// ---- a stage R <= 16: batches over the waves, inputs in registers (dft_batch of lfm_dft.hip with the general batch geometry)
template <int R, int CHW, bool INV, bool REAL_IN, bool REAL_OUT>
__device__ __forceinline__ void radix_stage(float2* __restrict__ tile, const float2* __restrict__ twR, const float2* __restrict__ twL, const Stage g,
                                            int lane, int wave) {
  constexpr int NW = (CHW == 64 ? 4 : 8);
  const int nb = g.P * g.Q;
  for (int b = wave; b < nb; b += NW) {
    const int kp = b / g.Q, jr = b - kp * g.Q;
    const int base = kp * R * g.Q + jr, k0 = kbase(g, kp);
    if (lane >= CHW) continue;
    float2 r[R];
#pragma unroll
    for (int j = 0; j < R; ++j) r[j] = tile[(base + j * g.Q) * CHW + lane];
    // (outputs go straight back to the batch's own slots: its inputs are all in registers by now)
    const int tstep = g.P * jr;                 // output k is multiplied by W_L^(P jr k): P jr k < L
#pragma unroll 2
    for (int k = 0; k < R; ++k) {
      if (g.last && k0 + g.P * k > g.kmax) break;
      const float2* __restrict__ row = twR + k * R;
      float2 t[R];
#pragma unroll
      for (int j = 1; j < R; ++j) t[j] = row[j];
      float2 acc = REAL_IN ? make_float2(r[0].x, 0.f) : r[0];
#pragma unroll
      for (int j = 1; j < R; ++j) {
        const float ty = INV ? -t[j].y : t[j].y;
        acc.x += r[j].x * t[j].x;
        if (!REAL_OUT) acc.y += r[j].x * ty;
        if (!REAL_IN) {
          acc.x -= r[j].y * ty;
          if (!REAL_OUT) acc.y += r[j].y * t[j].x;
        }
      }
      if (g.Q > 1 && k > 0) {
        float2 w = twL[tstep * k];
        if (INV) w.y = -w.y;
        acc = cmul(acc, w);
      }
      tile[(base + k * g.Q) * CHW + lane] = acc;
    }
  }
}

// ---- the stage of one prime p > 16: inputs from the tile, a wave's outputs in registers until the barrier, then in place.
// The sums of N units at once: per input j one tile read per unit and N * KB twiddles, all wave-uniform and independent of each other (no
// branch inside, so the scalar loads of one j go out together).  Twiddle of input j and output k0 + o: index
// mp (j (k0 + o) mod p) = (i0 + o jm) mod L with i0 = mp j k0 mod L and jm = mp j, each carried by add-and-wrap.
template <int N, int CHW, bool INV, bool REAL_IN, bool REAL_OUT>
__device__ __forceinline__ void direct_sums(const float2* __restrict__ tile, const float2* __restrict__ twL, int p, int L, int mp, int Q,
                                            const int (&base)[NU], const int (&k0)[NU], int ln, float2 (&acc)[NU][KB]) {
  int i0[N], s0[N];
#pragma unroll
  for (int u = 0; u < N; ++u) i0[u] = 0, s0[u] = mp * k0[u];      // k0 < p: below L
  int jm = 0;
  for (int j = 0; j < p; ++j) {
    float2 x[N];
#pragma unroll
    for (int u = 0; u < N; ++u) x[u] = tile[(base[u] + j * Q) * CHW + ln];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      int idx = i0[u];
#pragma unroll
      for (int o = 0; o < KB; ++o) {
        const float2 w = twL[idx];
        const float wy = INV ? -w.y : w.y;
        acc[u][o].x += x[u].x * w.x;
        if (!REAL_OUT) acc[u][o].y += x[u].x * wy;
        if (!REAL_IN) {
          acc[u][o].x -= x[u].y * wy;
          if (!REAL_OUT) acc[u][o].y += x[u].y * w.x;
        }
        idx += jm;
        if (idx >= L) idx -= L;
      }
      i0[u] += s0[u];
      if (i0[u] >= L) i0[u] -= L;
    }
    jm += mp;                                       // j < p: below L
  }
}

template <int CHW, bool INV, bool REAL_IN, bool REAL_OUT>
__device__ __forceinline__ void direct_stage(float2* __restrict__ tile, const float2* __restrict__ twL, int p, const Stage g, int lane, int wave) {
  constexpr int NW = (CHW == 64 ? 4 : 8);
  const int L = g.L, nb = g.P * g.Q, mp = L / p;     // W_p^x = W_L^(mp x)
  // outputs a batch needs: all p, or, in the last stage, those that can lie within the half spectrum (k0 + P k <= kmax for some k0 >= 0)
  const int need = g.last ? min(p, g.kmax / g.P + 1) : p;
  const int nkb = (need + KB - 1) / KB;             // units per batch: <= NW * NU because p <= 128 (CHW 64), 251 (CHW 32)
  const int bpr = (NW * NU) / nkb;                  // whole batches per round
  const bool act = lane < CHW;
  const int ln = act ? lane : 0;                    // (idle lanes read along with lane 0 and write nothing)
  for (int b0 = 0; b0 < nb; b0 += bpr) {
    // unit u of this wave is slot u * NW + wave of the round (consecutive units on different waves: a pruned batch keeps all waves busy);
    // the slots that hold work are a prefix in u
    float2 acc[NU][KB];
    int base[NU], k0[NU], nact = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int o = 0; o < KB; ++o) acc[u][o] = make_float2(0.f, 0.f);
      const int gi = u * NW + wave, bi = gi / nkb, b = b0 + bi;
      const bool on = bi < bpr && b < nb;
      const int kp = on ? b / g.Q : 0, jr = on ? b - kp * g.Q : 0;
      base[u] = kp * p * g.Q + jr;
      k0[u] = on ? (gi - bi * nkb) * KB : 0;
      nact += on ? 1 : 0;
    }
    switch (nact) {
      case 4: direct_sums<4, CHW, INV, REAL_IN, REAL_OUT>(tile, twL, p, L, mp, g.Q, base, k0, ln, acc); break;
      case 3: direct_sums<3, CHW, INV, REAL_IN, REAL_OUT>(tile, twL, p, L, mp, g.Q, base, k0, ln, acc); break;
      case 2: direct_sums<2, CHW, INV, REAL_IN, REAL_OUT>(tile, twL, p, L, mp, g.Q, base, k0, ln, acc); break;
      case 1: direct_sums<1, CHW, INV, REAL_IN, REAL_OUT>(tile, twL, p, L, mp, g.Q, base, k0, ln, acc); break;
      default: break;
    }
    static_assert(NU == 4, "the switch above lists the unit counts");
    __syncthreads();                                // every wave has read what it needs of this round's batches
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (u >= nact || !act) continue;
      const int b = b0 + (u * NW + wave) / nkb;
      const int kp = b / g.Q, jr = b - kp * g.Q;
      const int kb = kbase(g, kp), tstep = g.P * jr;
#pragma unroll
      for (int o = 0; o < KB; ++o) {
        const int k = k0[u] + o;
        if (k >= p || (g.last && kb + g.P * k > g.kmax)) continue;
        float2 v = acc[u][o];
        if (g.Q > 1 && k > 0) {
          float2 w = twL[tstep * k];
          if (INV) w.y = -w.y;
          v = cmul(v, w);
        }
        tile[(base[u] + k * g.Q) * CHW + lane] = v;
      }
    }
    if (b0 + bpr < nb) __syncthreads();             // the next round's batches are other slots, but keep the rounds apart
  }
}

#define OCPG_ANY_CASE(R_) case R_: radix_stage<R_, CHW, INV, REAL_IN, REAL_OUT>(tile, twR, twL, g, lane, wave); break;
template <int CHW, bool INV, bool REAL_IN, bool REAL_OUT>
__device__ __forceinline__ void any_stage(int R, float2* __restrict__ tile, const float2* __restrict__ twR, const float2* __restrict__ twL, const Stage g,
                                          int lane, int wave) {
  switch (R) {
    OCPG_ANY_CASE(2) OCPG_ANY_CASE(3) OCPG_ANY_CASE(4) OCPG_ANY_CASE(5) OCPG_ANY_CASE(6) OCPG_ANY_CASE(7) OCPG_ANY_CASE(8) OCPG_ANY_CASE(9)
    OCPG_ANY_CASE(10) OCPG_ANY_CASE(11) OCPG_ANY_CASE(12) OCPG_ANY_CASE(13) OCPG_ANY_CASE(14) OCPG_ANY_CASE(15) OCPG_ANY_CASE(16)
    default: direct_stage<CHW, INV, REAL_IN, REAL_OUT>(tile, twL, R, g, lane, wave); break;
  }
}
#undef OCPG_ANY_CASE

// Element j of the line sits at tile[j * CHW + channel] on entry; output element k sits at slot slots[k] on exit.  kmax: only outputs
// k <= kmax are needed (half spectrum of a real line).  REAL_IN holds for the first stage, REAL_OUT for the last (never both here).
template <int CHW, bool INV, bool REAL_IN = false, bool REAL_OUT = false>
__device__ __forceinline__ void line_dft(float2* __restrict__ tile, const Plan pl, const float2* __restrict__ tw, int lane, int wave, int kmax) {
  static_assert(!(REAL_IN && REAL_OUT), "one of them");
  int P = 1;
  for (int i = 0; i < pl.ns; ++i) {
    // (selects, not pl.s[i]: an array of the kernel argument indexed at run time would be copied to scratch)
    const int R = i == 0 ? pl.s[0] : i == 1 ? pl.s[1] : pl.s[2];
    Stage g;
    g.L = pl.L, g.P = P, g.Q = pl.L / (P * R), g.kmax = kmax, g.last = i == pl.ns - 1;
    g.kd = (g.last && pl.ns == 3) ? pl.s[1] : 1;
    const float2* __restrict__ twR = tw + (i == 0 ? pl.off[0] : i == 1 ? pl.off[1] : pl.off[2]);
    if (REAL_IN && i == 0) any_stage<CHW, INV, true, false>(R, tile, twR, tw, g, lane, wave);
    else if (REAL_OUT && g.last) any_stage<CHW, INV, false, true>(R, tile, twR, tw, g, lane, wave);
    else any_stage<CHW, INV, false, false>(R, tile, twR, tw, g, lane, wave);
    __syncthreads();
    P *= R;
  }
}

// ---- along w, real -> half spectrum.  grid (N*H, ceil(C / CHW)), 64 * NW threads
template <int CHW>
__global__ __launch_bounds__(CHW == 64 ? 256 : 512) void rows_fwd_any(const float* __restrict__ x, int W, int C, Plan pl, const float2* __restrict__ tw,
                                                                      float2* __restrict__ T) {
  extern __shared__ float2 tile[];
  constexpr int NT = (CHW == 64 ? 256 : 512), NR = NT / CHW;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int er = threadIdx.x / CHW, ch = threadIdx.x % CHW;
  const int* __restrict__ slots = (const int*)(tw + pl.slot);
  const long long line = blockIdx.x;
  const int c = blockIdx.y * CHW + ch;
  const bool ok = c < C;
  const int Wh = W / 2 + 1;
  for (int j0 = er; j0 < W; j0 += NR * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * NR;
      v[u] = (ok && j < W) ? x[(line * W + j) * C + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * NR;
      if (j < W) tile[j * CHW + ch] = make_float2(v[u], 0.f);
    }
  }
  __syncthreads();
  line_dft<CHW, false, true, false>(tile, pl, tw, lane, wave, W / 2);
  if (ok)
    for (int v = er; v < Wh; v += NR) T[(line * Wh + v) * C + c] = tile[slots[v] * CHW + ch];
}

// ---- along h, half spectrum -> gated [Re || Im] pair, both mirror halves.  grid (N * (W/2+1), ceil(C / CHW))
template <int CHW, typename P>
__global__ __launch_bounds__(CHW == 64 ? 256 : 512) void cols_fwd_any(const float2* __restrict__ T, const float* __restrict__ coef,
                                                                      const float* __restrict__ high, int H, int W, int C, Plan pl,
                                                                      const float2* __restrict__ tw, float norm, P* __restrict__ pair) {
  extern __shared__ float2 tile[];
  constexpr int NT = (CHW == 64 ? 256 : 512), NR = NT / CHW;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int er = threadIdx.x / CHW, ch = threadIdx.x % CHW;
  const int* __restrict__ slots = (const int*)(tw + pl.slot);
  const int Wh = W / 2 + 1;
  const int n = blockIdx.x / Wh, v = blockIdx.x - n * Wh;
  const int c = blockIdx.y * CHW + ch;
  const bool ok = c < C;
  for (int y0 = er; y0 < H; y0 += NR * U) {
    float2 q[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int y = y0 + i * NR;
      q[i] = (ok && y < H) ? T[(((long long)n * H + y) * Wh + v) * C + c] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int y = y0 + i * NR;
      if (y < H) tile[y * CHW + ch] = q[i];
    }
  }
  __syncthreads();
  line_dft<CHW, false>(tile, pl, tw, lane, wave, H);
  if (!ok) return;
  const float cf = coef ? coef[n] : 0.f;
  const int vm = W - v;                                   // the mirror column (v = 0 and v = W / 2 mirror onto themselves)
  const bool mirror = v > 0 && vm > v;
  for (int u = er; u < H; u += NR) {
    const float2 sv = tile[slots[u] * CHW + ch];
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
  }
}

// ---- pair (* gate) -> Hermitian part -> inverse along h.  grid (N * (W/2+1), ceil(C / CHW)); part [N][(W/2+1) * gridDim.y]
template <int CHW, typename P>
__global__ __launch_bounds__(CHW == 64 ? 256 : 512) void cols_inv_any(const P* __restrict__ pair, const float* __restrict__ coef,
                                                                      const float* __restrict__ high, const P* __restrict__ zs, float* __restrict__ part,
                                                                      int H, int W, int C, Plan pl, const float2* __restrict__ tw, float2* __restrict__ T) {
  extern __shared__ float2 tile[];
  constexpr int NT = (CHW == 64 ? 256 : 512), NR = NT / CHW, NW = NT / 64;
  __shared__ float red[NW];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int er = threadIdx.x / CHW, ch = threadIdx.x % CHW;
  const int* __restrict__ slots = (const int*)(tw + pl.slot);
  const int Wh = W / 2 + 1;
  const int n = blockIdx.x / Wh, v = blockIdx.x - n * Wh;
  const int c = blockIdx.y * CHW + ch;
  const bool ok = c < C;
  const float cf = coef ? coef[n] : 0.f;
  const int vm = v ? W - v : 0;
  float dsum = 0.f;
  constexpr int UI = 4;
  for (int u0 = er; u0 < H; u0 += NR * UI) {
    float ar[UI], ai[UI], br[UI], bi[UI], za[UI], zb[UI], zc[UI], zd[UI], ha[UI], hb[UI];
#pragma unroll
    for (int i = 0; i < UI; ++i) {
      const int u = u0 + i * NR;
      ar[i] = ai[i] = br[i] = bi[i] = za[i] = zb[i] = zc[i] = zd[i] = ha[i] = hb[i] = 0.f;
      if (ok && u < H) {
        const int um = u ? H - u : 0;
        const long long ia = (((long long)n * H + u) * W + v) * 2 * C + c, ib = (((long long)n * H + um) * W + vm) * 2 * C + c;
        ar[i] = ldf(pair + ia), ai[i] = ldf(pair + ia + C), br[i] = ldf(pair + ib), bi[i] = ldf(pair + ib + C);
        if (coef) ha[i] = high[u * W + v], hb[i] = high[um * W + vm];
        if (part) {
          za[i] = ldf(zs + ia), zb[i] = ldf(zs + ia + C);
          if (vm != v) zc[i] = ldf(zs + ib), zd[i] = ldf(zs + ib + C);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < UI; ++i) {
      const int u = u0 + i * NR;
      if (u >= H) continue;
      const float ga = 1.f - cf * ha[i], gb = 1.f - cf * hb[i];
      // d/dcoef of S * (1 - coef * high): -high * (g_re S_re + g_im S_im), with S = z / gate from the saved gated spectrum (a gate
      // of exactly 0 has lost S: that single term is dropped, as in lfm_dft.hip)
      if (part && ok) {
        if (ga != 0.f) dsum -= ha[i] * (ar[i] * za[i] + ai[i] * zb[i]) / ga;
        if (vm != v && gb != 0.f) dsum -= hb[i] * (br[i] * zc[i] + bi[i] * zd[i]) / gb;
      }
      tile[u * CHW + ch] = make_float2(0.5f * (ar[i] * ga + br[i] * gb), 0.5f * (ai[i] * ga - bi[i] * gb));
    }
  }
  __syncthreads();
  line_dft<CHW, true>(tile, pl, tw, lane, wave, H);
  if (ok)
    for (int y = er; y < H; y += NR) T[(((long long)n * H + y) * Wh + v) * C + c] = tile[slots[y] * CHW + ch];
  if (part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dsum += __shfl_down(dsum, o, 64);
    if (lane == 0) red[wave] = dsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
      for (int i = 0; i < NW; ++i) t += red[i];
      part[((long long)n * Wh + v) * gridDim.y + blockIdx.y] = t;
    }
  }
}

// ---- half spectrum -> real line (+ residual).  grid (N*H, ceil(C / CHW))
template <int CHW>
__global__ __launch_bounds__(CHW == 64 ? 256 : 512) void rows_inv_any(const float2* __restrict__ T, int W, int C, Plan pl, const float2* __restrict__ tw,
                                                                      float norm, const float* __restrict__ residual, float* __restrict__ out) {
  extern __shared__ float2 tile[];
  constexpr int NT = (CHW == 64 ? 256 : 512), NR = NT / CHW;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int er = threadIdx.x / CHW, ch = threadIdx.x % CHW;
  const int* __restrict__ slots = (const int*)(tw + pl.slot);
  const long long line = blockIdx.x;
  const int c = blockIdx.y * CHW + ch;
  const bool ok = c < C;
  const int Wh = W / 2 + 1;
  for (int v0 = er; v0 < W; v0 += NR * U) {
    float2 q[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int v = v0 + i * NR;
      q[i] = make_float2(0.f, 0.f);
      if (ok && v < W) q[i] = T[(line * Wh + (v < Wh ? v : W - v)) * C + c];
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int v = v0 + i * NR;
      if (v < W) tile[v * CHW + ch] = make_float2(q[i].x, v < Wh ? q[i].y : -q[i].y);
    }
  }
  __syncthreads();
  line_dft<CHW, true, false, true>(tile, pl, tw, lane, wave, W);
  if (ok)
    for (int j0 = er; j0 < W; j0 += NR * U) {
      float rs[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const int j = j0 + i * NR;
        rs[i] = (residual && j < W) ? residual[(line * W + j) * C + c] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const int j = j0 + i * NR;
        if (j < W) out[(line * W + j) * C + c] = norm * tile[slots[j] * CHW + ch].x + rs[i];
      }
    }
}

inline int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

inline int chw_of(int L) { return L > 128 ? 32 : 64; }

template <int CHW, typename P>
void launch_cols_fwd(const void* tmp, const float* coef, const float* high, int N, int H, int W, int C, const Plan& ph, const void* tw_h, float norm, void* pair,
                     hipStream_t st) {
  const dim3 g((unsigned)(N * (W / 2 + 1)), (C + CHW - 1) / CHW);
  cols_fwd_any<CHW, P><<<g, CHW == 64 ? 256 : 512, (size_t)H * CHW * sizeof(float2), st>>>((const float2*)tmp, coef, high, H, W, C, ph, (const float2*)tw_h, norm,
                                                                                         (P*)pair);
}

template <int CHW, typename P>
void launch_cols_inv(const void* pair, const float* coef, const float* high, const void* zs, float* part, int N, int H, int W, int C, const Plan& ph,
                     const void* tw_h, void* tmp, hipStream_t st) {
  const dim3 g((unsigned)(N * (W / 2 + 1)), (C + CHW - 1) / CHW);
  cols_inv_any<CHW, P><<<g, CHW == 64 ? 256 : 512, (size_t)H * CHW * sizeof(float2), st>>>((const P*)pair, coef, high, (const P*)zs, part, H, W, C, ph,
                                                                                         (const float2*)tw_h, (float2*)tmp);
}

}  // namespace
