// MSDeformAttn cross-attention with FEW queries: sample the UNPROJECTED tokens first, project afterwards.
//
// Bilinear sampling and the attention-weighted sum are linear in `value`, and value_proj is the same map for every token:
//
//   value      = masked_fill(src * Wv^T + bv, pad, 0)
//   out[q,h,:] = sum_k A_k sum_{c in V} w_c * value[pix_c, h, :]
//              = ( sum_k A_k sum_{c in V} w_c * src[pix_c, :] ) * Wv_h^T + ( sum_k A_k sum_{c in V} w_c ) * bv_h
//              =   s[q,h,:] * Wv_h^T + beta[q,h] * bv_h
//
// (V: corners inside the map and on tokens that are not padded; Wv_h: rows h*D .. h*D+D-1 of the weight.)  With Lq queries per image
// only 4*Lq*M*L*P rows of `value` are ever read; at the decoder's Lq = 5 against S = 5100 tokens that is 6 % of what value_proj writes,
// and the same share of grad_value's rows is all the weight- and input-gradient GEMMs do not multiply by zero.  Here the projection
// runs on the N*Lq*M sampled rows instead: no [N*S, C] x [C, C] GEMM forward, none backward, no dense grad_value.
//
//   msda_sf_fwd        one workgroup per (n, q, h), one thread per channel of the C-wide token: s, beta, then the D x C projection from LDS
//   msda_sf_bwd        same mapping: t = grad_out_h * Wv_h; per sample the three C-long dots behind grad_attn / grad_loc (wave shuffle +
//                      a fixed-order sum over the waves); grad_src += A * w * t by float atomics (coalesced 4*C-byte rows)
//   msda_sf_bwd_params grad_wv / grad_bv from grad_out, s and beta: one workgroup per weight row, fixed summation order, no atomics
//
// Corner validity and coordinates come from msda_dev.h's make_sample, as in every other MSDeformAttn kernel of this library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"
#include "msda_dev.h"

namespace {

constexpr int kMaxSamples = 64;   // L * P
constexpr int kMaxC = 1024;
constexpr int kThreads = 256;

using ocpg_dev::SampleRec;
using ocpg_dev::make_sample;

// Sample records of one (n, q, h) row over a C-wide token map; threads [0, NS) take one sample each.  A corner on a padded token is
// removed from the record's mask: it then counts neither in s nor in beta, exactly as masked_fill(value, pad, 0) makes it count.
__device__ __forceinline__ void setup_samples(const int64_t* __restrict__ shapes, const int64_t* __restrict__ level_start,
                                              const float* __restrict__ lrow, const float* __restrict__ arow,
                                              const unsigned char* __restrict__ padn, int P, int NS, int C, SampleRec* recs) {
  const int s = threadIdx.x;
  if (s < NS) {
    const int l = s / P;
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    SampleRec rec;
    make_sample<float>(lrow[2 * s], lrow[2 * s + 1], arow[s], H, W, (int)level_start[l], C, rec);
    if (padn && rec.mask) {
      const int pix = rec.off00 / C;       // exact: off00 is a multiple of C (also when the corner is virtual)
      const int dp[4] = {0, 1, W, W + 1};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((rec.mask & (1 << k)) && padn[pix + dp[k]]) rec.mask &= ~(1 << k);
    }
    recs[s] = rec;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// CPT channels per thread: thread t owns channels t, t + T, ... (T = blockDim.x = min(C, 256))
template <int CPT>
__global__ __launch_bounds__(kThreads) void msda_sf_fwd(const float* __restrict__ src, const float* __restrict__ wv,
                                                         const float* __restrict__ bv, const unsigned char* __restrict__ pad,
                                                         const int64_t* __restrict__ shapes, const int64_t* __restrict__ level_start,
                                                         const float* __restrict__ loc, const float* __restrict__ attn, int S, int M, int D,
                                                         int L, int Lq, int P, float* __restrict__ out, float* __restrict__ s_out,
                                                         float* __restrict__ beta_out) {
  __shared__ SampleRec recs[kMaxSamples];
  __shared__ float sv[kMaxC];
  const int C = M * D, NS = L * P, T = blockDim.x, tid = threadIdx.x;
  const long long row = blockIdx.x;              // flat (n, q, h)
  const int h = (int)(row % M);
  const long long nq = row / M;
  const long long n = nq / Lq;
  setup_samples(shapes, level_start, loc + row * NS * 2, attn + row * NS, pad ? pad + n * S : nullptr, P, NS, C, recs);
  __syncthreads();

  int ch[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) ch[i] = min(tid + i * T, C - 1);       // a thread past C re-reads the last channel and stores nothing
  const float* sb = src + n * (long long)S * C;
  float acc[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) acc[i] = 0.f;
  float beta = 0.f;
  // every load is issued whatever the corner's validity (from the map's first token when it is outside) and selected afterwards, so
  // the 4 * CPT loads of a sample -- and, unrolled, of its neighbours -- are in flight together
#pragma unroll 4
  for (int s = 0; s < NS; ++s) {
    const SampleRec rec = recs[s];
    const float hy = 1.f - rec.ly, hx = 1.f - rec.lx;
    const float w[4] = {hy * hx, hy * rec.lx, rec.ly * hx, rec.ly * rec.lx};
    const int offs[4] = {0, C, rec.rowstride, rec.rowstride + C};
    float v[4][CPT];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = (rec.mask >> k) & 1;
      const float* p = sb + (ok ? rec.off00 + offs[k] : 0);
#pragma unroll
      for (int i = 0; i < CPT; ++i) v[k][i] = p[ch[i]];
    }
    float wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = (rec.mask >> k) & 1;
      wsum += ok ? w[k] : 0.f;
#pragma unroll
      for (int i = 0; i < CPT; ++i) v[k][i] = ok ? v[k][i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i) acc[i] += (w[0] * v[0][i] + w[1] * v[1][i] + w[2] * v[2][i] + w[3] * v[3][i]) * rec.a;
    beta += wsum * rec.a;
  }
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = tid + i * T;
    if (c < C) {
      sv[c] = acc[i];
      s_out[row * C + c] = acc[i];
    }
  }
  if (tid == 0) beta_out[row] = beta;
  __syncthreads();
  // out[n, q, h*D + d] = s . Wv[h*D + d, :] + beta * bv[h*D + d]: one wave per output channel, lanes over the C-long weight row
  const int lane = tid & 63, wave = tid >> 6, nw = T >> 6;
  for (int d = wave; d < D; d += nw) {
    const float* wr = wv + (long long)(h * D + d) * C;
    float p = 0.f;
    for (int c = lane; c < C; c += 64) p += sv[c] * wr[c];
    p = wave_sum(p);
    if (lane == 0) out[nq * C + h * D + d] = p + (bv ? beta * bv[h * D + d] : 0.f);
  }
}

// SCATTER = false: grad_src is not wanted (NULL), only grad_loc / grad_attn are produced
template <int CPT, bool SCATTER>
__global__ __launch_bounds__(kThreads) void msda_sf_bwd(const float* __restrict__ src, const float* __restrict__ wv,
                                                         const float* __restrict__ bv, const unsigned char* __restrict__ pad,
                                                         const int64_t* __restrict__ shapes, const int64_t* __restrict__ level_start,
                                                         const float* __restrict__ loc, const float* __restrict__ attn,
                                                         const float* __restrict__ gout, int S, int M, int D, int L, int Lq, int P,
                                                         float* __restrict__ gsrc, float* __restrict__ gloc, float* __restrict__ gattn) {
  __shared__ SampleRec recs[kMaxSamples];
  __shared__ float red[kThreads / 64][kMaxSamples][3];
  const int C = M * D, NS = L * P, T = blockDim.x, tid = threadIdx.x;
  const long long row = blockIdx.x;              // flat (n, q, h)
  const int h = (int)(row % M);
  const long long nq = row / M;
  const long long n = nq / Lq;
  setup_samples(shapes, level_start, loc + row * NS * 2, attn + row * NS, pad ? pad + n * S : nullptr, P, NS, C, recs);

  int ch[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) ch[i] = min(tid + i * T, C - 1);
  // t = grad_out[n, q, h*D ..] . Wv_h (the gradient of the head's output w.r.t. a sampled, unprojected token), gb = grad_out_h . bv_h
  const float* go = gout + nq * C + h * D;
  float t[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) t[i] = 0.f;
  float gb = 0.f;
#pragma unroll 8
  for (int d = 0; d < D; ++d) {
    const float g = go[d];
    const float* wr = wv + (long long)(h * D + d) * C;
#pragma unroll
    for (int i = 0; i < CPT; ++i) t[i] += g * wr[ch[i]];
    if (bv) gb += g * bv[h * D + d];
  }
#pragma unroll
  for (int i = 0; i < CPT; ++i)
    if (tid + i * T >= C) t[i] = 0.f;           // a thread past C adds nothing to the dots
  __syncthreads();

  const float* sb = src + n * (long long)S * C;
  float* gs = SCATTER ? gsrc + n * (long long)S * C : nullptr;
  const int lane = tid & 63, wave = tid >> 6, nw = T >> 6;
  // GS samples at a time: all their corner rows are requested (from the map's first token where a corner is outside) before the first
  // is used, and their 3 * GS wave sums run side by side -- the workgroup is one of ~1.5 per CU, so latency is what it pays for
  constexpr int GS = CPT == 1 ? 4 : (CPT == 2 ? 2 : 1);
  for (int s0 = 0; s0 < NS; s0 += GS) {
    SampleRec rec[GS];
    float v[GS][4][CPT];
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      rec[u] = recs[min(s0 + u, NS - 1)];
      if (s0 + u >= NS) rec[u].mask = 0;
      const int offs[4] = {0, C, rec[u].rowstride, rec[u].rowstride + C};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = (rec[u].mask >> k) & 1;
        const float* p = sb + (ok ? rec[u].off00 + offs[k] : 0);
#pragma unroll
        for (int i = 0; i < CPT; ++i) v[u][k][i] = p[ch[i]];
      }
    }
    float part[GS][3];
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      const float hy = 1.f - rec[u].ly, hx = 1.f - rec[u].lx;
      const float w[4] = {hy * hx, hy * rec[u].lx, rec[u].ly * hx, rec[u].ly * rec[u].lx};
      const float dyc[4] = {-hx, -rec[u].lx, hx, rec[u].lx};
      const float dxc[4] = {-hy, hy, -rec[u].ly, rec[u].ly};
      const int offs[4] = {0, C, rec[u].rowstride, rec[u].rowstride + C};
      float pa = 0.f, px = 0.f, py = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((rec[u].mask >> k) & 1) {            // uniform across the workgroup
#pragma unroll
          for (int i = 0; i < CPT; ++i) {
            const float tv = t[i] * v[u][k][i];
            pa += w[k] * tv;
            px += dxc[k] * tv;
            py += dyc[k] * tv;
            if constexpr (SCATTER) {
              if (tid + i * T < C) atomicAdd(gs + rec[u].off00 + offs[k] + ch[i], w[k] * rec[u].a * t[i]);
            }
          }
        }
      }
      part[u][0] = pa;
      part[u][1] = px;
      part[u][2] = py;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < GS; ++u)
#pragma unroll
        for (int c = 0; c < 3; ++c) part[u][c] += __shfl_xor(part[u][c], o, 64);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < GS; ++u)
        if (s0 + u < NS) {                       // (a skipped sample's slot holds zeros the epilogue does not read)
          red[wave][s0 + u][0] = part[u][0];
          red[wave][s0 + u][1] = part[u][1];
          red[wave][s0 + u][2] = part[u][2];
        }
    }
  }
  __syncthreads();
  if (tid < NS) {
    const SampleRec rec = recs[tid];
    float ga = 0.f, gx = 0.f, gy = 0.f;
    if (rec.mask != 0) {
      for (int u = 0; u < nw; ++u) {
        ga += red[u][tid][0];
        gx += red[u][tid][1];
        gy += red[u][tid][2];
      }
      // the bias part of value: every valid corner carries bv_h on top of its projected token
      const float hy = 1.f - rec.ly, hx = 1.f - rec.lx;
      const float w[4] = {hy * hx, hy * rec.lx, rec.ly * hx, rec.ly * rec.lx};
      const float dyc[4] = {-hx, -rec.lx, hx, rec.lx};
      const float dxc[4] = {-hy, hy, -rec.ly, rec.ly};
      float ws = 0.f, xs = 0.f, ys = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((rec.mask >> k) & 1) {
          ws += w[k];
          xs += dxc[k];
          ys += dyc[k];
        }
      ga += gb * ws;
      gx = rec.W * rec.a * (gx + gb * xs);
      gy = rec.H * rec.a * (gy + gb * ys);
    }
    gattn[row * NS + tid] = ga;
    *reinterpret_cast<float2*>(gloc + (row * NS + tid) * 2) = make_float2(gx, gy);
  }
}

// grad_wv[o, c] = sum_r grad_out[r, o] * s[r, h, c], grad_bv[o] = sum_r grad_out[r, o] * beta[r, h]  (o = h*D + d, r over the N*Lq queries)
template <int CPT>
__global__ __launch_bounds__(kThreads) void msda_sf_bwd_params(const float* __restrict__ gout, const float* __restrict__ s_in,
                                                                const float* __restrict__ beta_in, long long R, int M, int D,
                                                                float* __restrict__ gwv, float* __restrict__ gbv) {
  const int C = M * D, T = blockDim.x, tid = threadIdx.x;
  const int o = blockIdx.x, h = o / D;
  int ch[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) ch[i] = min(tid + i * T, C - 1);
  float acc[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) acc[i] = 0.f;
  float b = 0.f;
#pragma unroll 4
  for (long long r = 0; r < R; ++r) {
    const float g = gout[r * C + o];
    const float* sr = s_in + (r * M + h) * C;
#pragma unroll
    for (int i = 0; i < CPT; ++i) acc[i] += g * sr[ch[i]];
    b += g * beta_in[r * M + h];
  }
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = tid + i * T;
    if (c < C) gwv[(long long)o * C + c] = acc[i];
  }
  if (gbv && tid == 0) gbv[o] = b;
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what the three kernels serve; everything else is the caller's value_proj + ocpg_msda_fwd_f32 / _bwd_f32
inline bool shape_ok(long long S, int M, int D, int L, int P) {
  const long long C = (long long)M * D;
  return C % 64 == 0 && C <= kMaxC && (long long)L * P <= kMaxSamples && S * C < (1LL << 31);
}

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

inline int check_dims(int N, int S, int M, int D, int L, int Lq, int P) {
  if (N < 0) return -1009;
  if (S <= 0) return -1010;
  if (M <= 0) return -1011;
  if (D <= 0) return -1012;
  if (L <= 0) return -1013;
  if (Lq < 0) return -1014;
  if (P <= 0) return -1015;
  return 0;
}

#define SF_DISPATCH(CPT_, ...)        \
  switch (CPT_) {                     \
    case 1: SF_LAUNCH(1, __VA_ARGS__); break; \
    case 2: SF_LAUNCH(2, __VA_ARGS__); break; \
    case 3: SF_LAUNCH(3, __VA_ARGS__); break; \
    default: SF_LAUNCH(4, __VA_ARGS__); break; \
  }

}  // namespace

extern "C" {

int ocpg_msda_sf_fwd_f32(const float* src, const float* wv, const float* bv, const unsigned char* pad, const int64_t* shapes,
                         const int64_t* level_start, const float* loc, const float* attn, int N, int S, int M, int D, int L, int Lq, int P,
                         float* out, float* s, float* beta, void* stream) {
  if (int e = check_dims(N, S, M, D, L, Lq, P)) return e;
  if (!shape_ok(S, M, D, L, P)) return -2000;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!src) return -1001;
  if (!wv) return -1002;
  if (!shapes) return -1005;
  if (!level_start) return -1006;
  if (!loc) return -1007;
  if (!attn) return -1008;
  if (!out) return -1016;
  if (!s) return -1017;
  if (!beta) return -1018;
  if (rows >= (1LL << 31)) return -2000;
  if (!aligned_to(src, 4) || !aligned_to(wv, 4) || !aligned_to(bv, 4) || !aligned_to(shapes, 8) || !aligned_to(level_start, 8) ||
      !aligned_to(loc, 4) || !aligned_to(attn, 4) || !aligned_to(out, 4) || !aligned_to(s, 4) || !aligned_to(beta, 4))
    return -2000;
  const int C = M * D, T = C < kThreads ? C : kThreads, cpt = (C + kThreads - 1) / kThreads;
  hipStream_t st = (hipStream_t)stream;
#define SF_LAUNCH(CPT_, ...) msda_sf_fwd<CPT_><<<(unsigned)rows, T, 0, st>>>(__VA_ARGS__)
  SF_DISPATCH(cpt, src, wv, bv, pad, shapes, level_start, loc, attn, S, M, D, L, Lq, P, out, s, beta)
#undef SF_LAUNCH
  return launch_status();
}

int ocpg_msda_sf_bwd_f32(const float* src, const float* wv, const float* bv, const unsigned char* pad, const int64_t* shapes,
                         const int64_t* level_start, const float* loc, const float* attn, const float* grad_out, int N, int S, int M,
                         int D, int L, int Lq, int P, float* grad_src, float* grad_loc, float* grad_attn, void* stream) {
  if (int e = check_dims(N, S, M, D, L, Lq, P)) return e - 1;
  if (!shape_ok(S, M, D, L, P)) return -2000;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!src) return -1001;
  if (!wv) return -1002;
  if (!shapes) return -1005;
  if (!level_start) return -1006;
  if (!loc) return -1007;
  if (!attn) return -1008;
  if (!grad_out) return -1009;
  if (!grad_loc) return -1018;
  if (!grad_attn) return -1019;
  if (rows >= (1LL << 31)) return -2000;
  if (!aligned_to(src, 4) || !aligned_to(wv, 4) || !aligned_to(bv, 4) || !aligned_to(shapes, 8) || !aligned_to(level_start, 8) ||
      !aligned_to(loc, 4) || !aligned_to(attn, 4) || !aligned_to(grad_out, 4) || !aligned_to(grad_src, 4) || !aligned_to(grad_loc, 8) ||
      !aligned_to(grad_attn, 4))
    return -2000;
  const int C = M * D, T = C < kThreads ? C : kThreads, cpt = (C + kThreads - 1) / kThreads;
  hipStream_t st = (hipStream_t)stream;
#define SF_LAUNCH(CPT_, ...)                                                          \
  if (grad_src) msda_sf_bwd<CPT_, true><<<(unsigned)rows, T, 0, st>>>(__VA_ARGS__);   \
  else msda_sf_bwd<CPT_, false><<<(unsigned)rows, T, 0, st>>>(__VA_ARGS__)
  SF_DISPATCH(cpt, src, wv, bv, pad, shapes, level_start, loc, attn, grad_out, S, M, D, L, Lq, P, grad_src, grad_loc, grad_attn)
#undef SF_LAUNCH
  return launch_status();
}

int ocpg_msda_sf_bwd_params_f32(const float* grad_out, const float* s, const float* beta, int N, int M, int D, int Lq, float* grad_wv,
                                float* grad_bv, void* stream) {
  if (N < 0) return -1004;
  if (M <= 0) return -1005;
  if (D <= 0) return -1006;
  if (Lq < 0) return -1007;
  if (!shape_ok(1, M, D, 1, 1)) return -2000;
  if (!grad_wv) return -1008;
  const long long R = (long long)N * Lq;
  if (R > 0) {
    if (!grad_out) return -1001;
    if (!s) return -1002;
    if (!beta) return -1003;
  }
  if (!aligned_to(grad_out, 4) || !aligned_to(s, 4) || !aligned_to(beta, 4) || !aligned_to(grad_wv, 4) || !aligned_to(grad_bv, 4)) return -2000;
  const int C = M * D, T = C < kThreads ? C : kThreads, cpt = (C + kThreads - 1) / kThreads;
  hipStream_t st = (hipStream_t)stream;
#define SF_LAUNCH(CPT_, ...) msda_sf_bwd_params<CPT_><<<(unsigned)C, T, 0, st>>>(__VA_ARGS__)
  SF_DISPATCH(cpt, grad_out, s, beta, R, M, D, grad_wv, grad_bv)
#undef SF_LAUNCH
  return launch_status();
}

}  // extern "C"
