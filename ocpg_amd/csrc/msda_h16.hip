// MSDeformAttn with 16-bit STORAGE of value / out / grad_out (bfloat16 or float16) for MI355X (gfx950, wave64).
//
// Counterparts of the fp32 row kernels of msda.hip, in a translation unit of their own so that the fp32 kernels' code generation
// cannot move.  What stays fp32: the sampling locations, the attention weights, their gradients, grad_value (atomic accumulation:
// there are no 16-bit atomics here) and ALL arithmetic; a 16-bit element is widened right after its load and `out` is rounded to
// nearest-even once, at its store.
//
// Lane mapping: a row (batch, query, head) is served by G lanes of CPL channels each, D = G * CPL.
//   CPL = 4: the fp32 kernels' lane structure (G = D / 4, DPP reduce-scatter over 8 lanes unchanged), 8-byte corner loads;
//   CPL = 8: 16-byte corner loads as in fp32 (G = D / 8: for D = 32 four lanes per row, 16 rows per wave), half the load
//            instructions per sample; the gather's sums over the row's lanes then stay inside a DPP quad.
// Both exist for the forward and the gather, un-fused and with the module's front end fused in (msda_fwd_fused_h16 /
// msda_bwd_gather_fused_h16: D = 32, L * P = 16); OCPG_MSDA_H16_LANES=4|8 forces one (A/B timing: tools/bench_msda_h16.py), the defaults
// below are what DESIGN.md section 4.3b records.
//
// The grad_value half of the self-attention backward reuses the column-scatter / output-tiled kernels (msda_col.hip, msda_tile.hip),
// which read grad_out at one site each and are templated on its storage type.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "../../include/ocpg_hip.h"
#include "msda_col.h"
#include "msda_dev.h"
#include "msda_host.h"

namespace {

using ocpg_dev::bf16s;
using ocpg_dev::fp16s;
using ocpg_dev::ld1;
using ocpg_dev::ld4;
using ocpg_dev::ldc;
using ocpg_dev::SampleRec;
using ocpg_dev::make_sample;
using ocpg_dev::GatherRec;
using ocpg_dev::make_gather;
using ocpg_dev::ldraw;
using ocpg_dev::widen;
using ocpg_dev::st1;
using ocpg_dev::stc;
using ocpg_dev::group_sum;
using ocpg_dev::dpp_xor1;
using ocpg_dev::dpp_xor2;
using ocpg_dev::reduce_scatter_g8_p4;

constexpr int kMaxLevels = 16;
#ifndef MSDA_H16_FWD_CPL
#define MSDA_H16_FWD_CPL 8          // default channels per lane of the forward  (measured: DESIGN.md section 4.3b)
#endif
#ifndef MSDA_H16_GATHER_CPL
#define MSDA_H16_GATHER_CPL 8       // ... and of the gather half of the backward
#endif

// sum over the G lanes of a row: inside a DPP quad for G <= 4 (no LDS crossbar)
template <int G>
__device__ __forceinline__ float row_sum(float v) {
  if constexpr (G == 1) return v;
  else if constexpr (G == 2) return v + dpp_xor1(v);
  else if constexpr (G == 4) { v += dpp_xor1(v); return v + dpp_xor2(v); }
  else return group_sum<G>(v);
}

// ------------------------------------------------------------------------------------------------------
// Fast forward: D = CPL * G, G a power of two <= 64.  256 threads = 256 / G rows per block.  LDS: rows * NS * 32 B (dynamic).
template <typename H, int G, int CPL>
__global__ __launch_bounds__(256) void msda_fwd_h16(const H* __restrict__ value, const int64_t* __restrict__ shapes,
                                                    const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                    const float* __restrict__ attn, int S, int M, int L, int Lq, int P,
                                                    long long rows, H* __restrict__ out) {
  constexpr int D = CPL * G;
  constexpr int ROWS = 256 / G;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  SampleRec* recs = reinterpret_cast<SampleRec*>(smem);
  __shared__ int lvlH[kMaxLevels], lvlW[kMaxLevels], lvlS[kMaxLevels];
  const int tid = threadIdx.x;
  if (tid < L) {
    lvlH[tid] = (int)shapes[2 * tid];
    lvlW[tid] = (int)shapes[2 * tid + 1];
    lvlS[tid] = (int)level_start[tid];
  }
  __syncthreads();
  const int NS = L * P;
  const int MD = M * D;
  const int r = tid / G, j = tid % G;
  // head fastest: blocks are dealt round-robin over the 8 XCDs, so with M == 8 every XCD gathers one head's slices through its own L2
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // flat (b, q)
  const long long row = qrow * M + (blockIdx.x % M);
  const bool live = qrow * M < rows;
  if (live) {
    const float* lrow = loc + row * NS * 2;
    const float* arow = attn + row * NS;
    for (int s = j; s < NS; s += G) {
      const int l = s / P;
      SampleRec rec;
      make_sample(lrow[2 * s], lrow[2 * s + 1], arow[s], lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + s] = rec;
    }
  }
  __syncthreads();
  if (!live) return;
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const H* vbase = value + b * (long long)S * MD + m * D + CPL * j;
  float acc[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc[c] = 0.f;
  const SampleRec* rr = recs + r * NS;
  for (int s = 0; s < NS; ++s) {
    const SampleRec rec = rr[s];
    if (rec.mask == 0) continue;  // uniform across the row's lanes
    const float hy = 1.f - rec.ly, hx = 1.f - rec.lx;
    // every corner is loaded (an outside corner from the row's own first pixel, always valid) and masked: four loads in flight, one wait
    // (msda_dev.h: ldraw / keep / widen)
    const unsigned m1 = (rec.mask & 1) ? ~0u : 0u, m2 = (rec.mask & 2) ? ~0u : 0u, m3 = (rec.mask & 4) ? ~0u : 0u, m4 = (rec.mask & 8) ? ~0u : 0u;
    const int o1 = rec.off00 & (int)m1, o2 = (rec.off00 + MD) & (int)m2, o3 = (rec.off00 + rec.rowstride) & (int)m3,
              o4 = (rec.off00 + rec.rowstride + MD) & (int)m4;
    const auto r1 = ocpg_dev::keep(ldraw<CPL>(vbase + o1), m1), r2 = ocpg_dev::keep(ldraw<CPL>(vbase + o2), m2),
               r3 = ocpg_dev::keep(ldraw<CPL>(vbase + o3), m3), r4 = ocpg_dev::keep(ldraw<CPL>(vbase + o4), m4);
    float v1[CPL], v2[CPL], v3[CPL], v4[CPL];
    widen(r1, vbase, v1); widen(r2, vbase, v2); widen(r3, vbase, v3); widen(r4, vbase, v4);
    const float w1 = hy * hx, w2 = hy * rec.lx, w3 = rec.ly * hx, w4 = rec.ly * rec.lx;
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] += (w1 * v1[c] + w2 * v2[c] + w3 * v3[c] + w4 * v4[c]) * rec.a;
  }
  stc<CPL>(out + row * D + CPL * j, acc);
}

// Generic forward: one wave per row, lanes stride over channels.  Any D.
template <typename H>
__global__ __launch_bounds__(256) void msda_fwd_generic_h16(const H* __restrict__ value, const int64_t* __restrict__ shapes,
                                                            const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                            const float* __restrict__ attn, int S, int M, int D, int L, int Lq, int P,
                                                            long long rows, H* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int NS = L * P;
  const long long MD = (long long)M * D;
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const H* vb = value + b * (long long)S * MD + (long long)m * D;
  for (int c = lane; c < D; c += 64) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) {
      const int Hh = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
      const long long ls = level_start[l];
      for (int p = 0; p < P; ++p) {
        const long long wi = row * NS + (long long)l * P + p;
        const float w_im = loc[2 * wi] * (float)W - 0.5f, h_im = loc[2 * wi + 1] * (float)Hh - 0.5f;
        if (!(h_im > -1.f && w_im > -1.f && h_im < (float)Hh && w_im < (float)W)) continue;
        const int y0 = (int)floorf(h_im), x0 = (int)floorf(w_im);
        const float ly = h_im - (float)y0, lx = w_im - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        const H* p00 = vb + (ls + (long long)y0 * W + x0) * MD + c;
        const bool y0ok = y0 >= 0, y1ok = y0 + 1 <= Hh - 1, x0ok = x0 >= 0, x1ok = x0 + 1 <= W - 1;
        const float v1 = (y0ok && x0ok) ? ld1(p00) : 0.f;
        const float v2 = (y0ok && x1ok) ? ld1(p00 + MD) : 0.f;
        const float v3 = (y1ok && x0ok) ? ld1(p00 + (long long)W * MD) : 0.f;
        const float v4 = (y1ok && x1ok) ? ld1(p00 + (long long)W * MD + MD) : 0.f;
        acc += (hy * hx * v1 + hy * lx * v2 + ly * hx * v3 + ly * lx * v4) * attn[wi];
      }
    }
    st1(out + row * D + c, acc);
  }
}

// ------------------------------------------------------------------------------------------------------
// Gather half of the backward (grad_loc, grad_attn), used with the column-scatter / output-tiled grad_value kernels: the 16-bit
// counterpart of msda_bwd_gather_row (validity folded into the per-axis weights, corner addresses clamped into the map: four
// unconditional loads per sample; four samples reduced together).  D is a multiple of 16 (the record packs four flag bits under an
// element offset that is a multiple of M * D).

template <typename H, int G, int CPL>
__global__ __launch_bounds__(256) void msda_bwd_gather_h16(const H* __restrict__ value, const int64_t* __restrict__ shapes,
                                                           const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                           const float* __restrict__ attn, const H* __restrict__ gout, int S, int M,
                                                           int L, int Lq, int P, long long rows, float* __restrict__ gloc,
                                                           float* __restrict__ gattn) {
  constexpr int D = CPL * G;
  static_assert(D % 16 == 0, "GatherRec packs 4 flag bits under the element offset");
  constexpr int ROWS = 256 / G;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  GatherRec* recs = reinterpret_cast<GatherRec*>(smem);
  __shared__ int lvlH[kMaxLevels], lvlW[kMaxLevels], lvlS[kMaxLevels];
  const int tid = threadIdx.x;
  if (tid < L) {
    lvlH[tid] = (int)shapes[2 * tid];
    lvlW[tid] = (int)shapes[2 * tid + 1];
    lvlS[tid] = (int)level_start[tid];
  }
  __syncthreads();
  const int NS = L * P;
  const int MD = M * D;
  const int r = tid / G, j = tid % G;
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // head fastest: one head per XCD L2
  const long long row = qrow * M + (blockIdx.x % M);
  const bool live = qrow * M < rows;
  if (live) {
    const float* lrow = loc + row * NS * 2;
    const float* arow = attn + row * NS;
    for (int s = j; s < NS; s += G) {
      const int l = s / P;
      GatherRec rec;
      make_gather(lrow[2 * s], lrow[2 * s + 1], arow[s], lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + s] = rec;
    }
  }
  __syncthreads();
  if (!live) return;  // whole row groups leave together (G divides 64): the DPP exchanges below stay within live groups
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const H* vbase = value + b * (long long)S * MD + m * D + CPL * j;
  float go[CPL];
  ldc<CPL>(gout + row * D + CPL * j, go);
  const GatherRec* rr = recs + r * NS;
  constexpr int NB = 4;
  auto batch = [&](const int s0) {
    float red[NB][3];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const bool have = s0 + i < NS;
      const GatherRec rec = rr[have ? s0 + i : s0];
      const int bits = rec.pk & 15;
      const H* p00 = vbase + (rec.pk & ~15);
      const int dx = (bits & 3) == 3 ? MD : 0, dy = (bits & 12) == 12 ? rec.rowstride : 0;
      float v0[CPL], v1[CPL], v2[CPL], v3[CPL];
      ldc<CPL>(p00, v0); ldc<CPL>(p00 + dx, v1); ldc<CPL>(p00 + dy, v2); ldc<CPL>(p00 + dy + dx, v3);
      // per-corner dot products with the output gradient first: the weights then act on 4 scalars, not on 4 x D channels
      float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
      for (int c = 0; c < CPL; ++c) { d0 += go[c] * v0[c]; d1 += go[c] * v1[c]; d2 += go[c] * v2[c]; d3 += go[c] * v3[c]; }
      const float ix0 = (bits & 1) ? 1.f : 0.f, ix1 = (bits & 2) ? 1.f : 0.f, iy0 = (bits & 4) ? 1.f : 0.f, iy1 = (bits & 8) ? 1.f : 0.f;
      const float top = rec.hx * d0 + rec.lx * d1, bot = rec.hx * d2 + rec.lx * d3;          // rows ya / yb, x-interpolated
      const float lef = ix1 * d1 - ix0 * d0, rig = ix1 * d3 - ix0 * d2;                      // d/dx along rows ya / yb
      const float ga = rec.hy * top + rec.ly * bot;
      const float gx = rec.aW * (rec.hy * lef + rec.ly * rig);
      const float gy = rec.aH * (iy1 * bot - iy0 * top);
      red[i][0] = have ? ga : 0.f;
      red[i][1] = have ? gx : 0.f;
      red[i][2] = have ? gy : 0.f;
    }
    if (G == 8 && s0 + NB <= NS) {
      float tot[3];
      const int sidx = reduce_scatter_g8_p4(red, j, tot);
      if ((j & 1) == 0) {
        const long long wi = row * NS + s0 + sidx;
        gattn[wi] = tot[0];
        *reinterpret_cast<float2*>(gloc + wi * 2) = make_float2(tot[1], tot[2]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        if (s0 + i >= NS) continue;
        const float ga = row_sum<G>(red[i][0]), gx = row_sum<G>(red[i][1]), gy = row_sum<G>(red[i][2]);
        if (j == (G <= 4 ? i % G : 0)) {       // (quads: every lane holds the totals, so the four stores of a batch spread over the lanes)
          const long long wi = row * NS + s0 + i;
          gattn[wi] = ga;
          *reinterpret_cast<float2*>(gloc + wi * 2) = make_float2(gx, gy);
        }
      }
    }
  };
#pragma unroll 1
  for (int s0 = 0; s0 < NS; s0 += NB) batch(s0);
}

// ------------------------------------------------------------------------------------------------------
// Whole backward of a row with a plain fp32 atomic scatter for grad_value (cross-attention, Lq != S): D = 4 * G.
template <typename H, int G>
__global__ __launch_bounds__(256) void msda_bwd_row_h16(const H* __restrict__ value, const int64_t* __restrict__ shapes,
                                                        const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                        const float* __restrict__ attn, const H* __restrict__ gout, int S, int M,
                                                        int L, int Lq, int P, long long rows, float* __restrict__ gvalue,
                                                        float* __restrict__ gloc, float* __restrict__ gattn) {
  constexpr int D = 4 * G;
  constexpr int ROWS = 256 / G;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  SampleRec* recs = reinterpret_cast<SampleRec*>(smem);
  __shared__ int lvlH[kMaxLevels], lvlW[kMaxLevels], lvlS[kMaxLevels];
  const int tid = threadIdx.x;
  if (tid < L) {
    lvlH[tid] = (int)shapes[2 * tid];
    lvlW[tid] = (int)shapes[2 * tid + 1];
    lvlS[tid] = (int)level_start[tid];
  }
  __syncthreads();
  const int NS = L * P;
  const int MD = M * D;
  const int r = tid / G, j = tid % G;
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // flat (b, q); head = block % M
  const long long row = qrow * M + (blockIdx.x % M);
  const bool live = qrow * M < rows;
  if (live) {
    const float* lrow = loc + row * NS * 2;
    const float* arow = attn + row * NS;
    for (int s = j; s < NS; s += G) {
      const int l = s / P;
      SampleRec rec;
      make_sample(lrow[2 * s], lrow[2 * s + 1], arow[s], lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + s] = rec;
    }
  }
  __syncthreads();
  if (!live) return;  // whole row groups leave together (G divides 64): shuffles below stay within live groups
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const H* vbase = value + b * (long long)S * MD + m * D + 4 * j;
  float* gsc = gvalue + b * (long long)S * MD + m * D + j;
  const float4 go = ld4(gout + row * D + 4 * j);
  // scatter: lane j owns channels {j, j+G, j+2G, j+3G}, so one atomic instruction covers G consecutive floats of the row
  const float gs[4] = {ld1(gout + row * D + j), ld1(gout + row * D + j + G), ld1(gout + row * D + j + 2 * G), ld1(gout + row * D + j + 3 * G)};
  const SampleRec* rr = recs + r * NS;
  for (int s = 0; s < NS; ++s) {
    const SampleRec rec = rr[s];
    float ga = 0.f, gx = 0.f, gy = 0.f;
    if (rec.mask != 0) {
      const float hy = 1.f - rec.ly, hx = 1.f - rec.lx;
      const float w[4] = {hy * hx, hy * rec.lx, rec.ly * hx, rec.ly * rec.lx};
      const float dyc[4] = {-hx, -rec.lx, hx, rec.lx};
      const float dxc[4] = {-hy, hy, -rec.ly, rec.ly};
      const int offs[4] = {0, MD, rec.rowstride, rec.rowstride + MD};
      const float4 tg = make_float4(go.x * rec.a, go.y * rec.a, go.z * rec.a, go.w * rec.a);  // top_grad * attn_weight
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 dxs = val, dys = val;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (rec.mask & (1 << k)) {
          const float4 v = ld4(vbase + rec.off00 + offs[k]);
          float* g = gsc + rec.off00 + offs[k];
#pragma unroll
          for (int c = 0; c < 4; ++c) atomicAdd(g + c * G, w[k] * gs[c] * rec.a);
          val.x += w[k] * v.x; val.y += w[k] * v.y; val.z += w[k] * v.z; val.w += w[k] * v.w;
          dxs.x += dxc[k] * v.x; dxs.y += dxc[k] * v.y; dxs.z += dxc[k] * v.z; dxs.w += dxc[k] * v.w;
          dys.x += dyc[k] * v.x; dys.y += dyc[k] * v.y; dys.z += dyc[k] * v.z; dys.w += dyc[k] * v.w;
        }
      }
      ga = go.x * val.x + go.y * val.y + go.z * val.z + go.w * val.w;
      gx = rec.W * (dxs.x * tg.x + dxs.y * tg.y + dxs.z * tg.z + dxs.w * tg.w);
      gy = rec.H * (dys.x * tg.x + dys.y * tg.y + dys.z * tg.z + dys.w * tg.w);
    }
    ga = group_sum<G>(ga);
    gx = group_sum<G>(gx);
    gy = group_sum<G>(gy);
    if (j == 0) {
      gattn[row * NS + s] = ga;
      *reinterpret_cast<float2*>(gloc + (row * NS + s) * 2) = make_float2(gx, gy);
    }
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Generic backward: one wave per row; any D.
template <typename H>
__global__ __launch_bounds__(256) void msda_bwd_generic_h16(const H* __restrict__ value, const int64_t* __restrict__ shapes,
                                                            const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                            const float* __restrict__ attn, const H* __restrict__ gout, int S, int M, int D,
                                                            int L, int Lq, int P, long long rows, float* __restrict__ gvalue,
                                                            float* __restrict__ gloc, float* __restrict__ gattn) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int NS = L * P;
  const long long MD = (long long)M * D;
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const long long boff = b * (long long)S * MD + (long long)m * D;
  for (int l = 0; l < L; ++l) {
    const int Hh = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    const long long ls = level_start[l];
    for (int p = 0; p < P; ++p) {
      const long long wi = row * NS + (long long)l * P + p;
      const float w_im = loc[2 * wi] * (float)W - 0.5f, h_im = loc[2 * wi + 1] * (float)Hh - 0.5f;
      float ga = 0.f, gx = 0.f, gy = 0.f;
      if (h_im > -1.f && w_im > -1.f && h_im < (float)Hh && w_im < (float)W) {
        const int y0 = (int)floorf(h_im), x0 = (int)floorf(w_im);
        const float ly = h_im - (float)y0, lx = w_im - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        const float a = attn[wi];
        const bool ok[4] = {y0 >= 0 && x0 >= 0, y0 >= 0 && x0 + 1 <= W - 1, y0 + 1 <= Hh - 1 && x0 >= 0,
                            y0 + 1 <= Hh - 1 && x0 + 1 <= W - 1};
        const float w[4] = {hy * hx, hy * lx, ly * hx, ly * lx};
        const float dyc[4] = {-hx, -lx, hx, lx};
        const float dxc[4] = {-hy, hy, -ly, ly};
        const long long o00 = boff + (ls + (long long)y0 * W + x0) * MD;
        const long long offs[4] = {0, MD, (long long)W * MD, (long long)W * MD + MD};
        for (int c = lane; c < D; c += 64) {
          const float tg = ld1(gout + row * D + c);
          const float tga = tg * a;
          float val = 0.f, dx = 0.f, dy = 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (ok[k]) {
              const float v = ld1(value + o00 + offs[k] + c);
              atomicAdd(gvalue + o00 + offs[k] + c, w[k] * tga);
              val += w[k] * v;
              dx += dxc[k] * v;
              dy += dyc[k] * v;
            }
          }
          ga += tg * val;
          gx += (float)W * dx * tga;
          gy += (float)Hh * dy * tga;
        }
      }
      ga = wave_sum(ga);
      gx = wave_sum(gx);
      gy = wave_sum(gy);
      if (lane == 0) {
        gattn[wi] = ga;
        gloc[2 * wi] = gx;
        gloc[2 * wi + 1] = gy;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// Fused front end (include/ocpg_hip.h: ocpg_msda_fused_*_h16): the 16-bit counterparts of msda_fwd_fused8 and
// msda_bwd_gather_row<8, true> of msda.hip.  D = 32, L * P = 16; G = 4 lanes of 8 channels (default) or G = 8 lanes of 4.
//
// Sum 4 samples x {ga, gx, gy} over the 4 lanes of a row as a reduce-scatter inside the DPP quad: after it lane j holds sample j's
// three totals (9 DPP moves; the all-reduce of row_sum<4> would take 24 and leave every lane with values three of them drop).
__device__ __forceinline__ void reduce_scatter_g4_p4(const float (&v)[4][3], int j, float (&out)[3]) {
  const bool hi = (j & 2) != 0;          // step 1: partner j^2; keep samples {0,1} or {2,3}
  float a[2][3];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float keep = hi ? v[2 + s][c] : v[s][c];
      const float send = hi ? v[s][c] : v[2 + s][c];
      a[s][c] = keep + dpp_xor2(send);
    }
  const bool lo = (j & 1) != 0;          // step 2: partner j^1; keep sample 0 or 1 of the pair
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float keep = lo ? a[1][c] : a[0][c];
    const float send = lo ? a[0][c] : a[1][c];
    out[c] = keep + dpp_xor1(send);
  }
}

template <int G>
__device__ __forceinline__ float row_max(float v) {
  if constexpr (G == 4) {
    v = fmaxf(v, dpp_xor1(v));
    return fmaxf(v, dpp_xor2(v));
  } else {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  }
}

// Fused forward.  qproj [N*Lq, 3*M*16] = [offsets (M, L, P, 2), already divided by (W_l, H_l) | logits (M, 16)], ref [N*Lq, L, 2]: lane j
// of a row owns the samples j, j + G, ... in the set-up (softmax over the 16 logits, reference + offset, loc_out / attn_out written in
// fp32, the sample records); the sampling loop is msda_fwd_h16's.
template <typename H, int G, int CPL>
__global__ __launch_bounds__(256) void msda_fwd_fused_h16(const H* __restrict__ value, const int64_t* __restrict__ shapes,
                                                          const int64_t* __restrict__ level_start, const float* __restrict__ qproj,
                                                          const float* __restrict__ ref, int S, int M, int L, int Lq, int P, long long rows,
                                                          H* __restrict__ out, float* __restrict__ loc_out, float* __restrict__ attn_out) {
  constexpr int D = CPL * G, ROWS = 256 / G, NS = 16, U = NS / G;
  static_assert(D == 32 && (G == 4 || G == 8), "D = 32 as 4 x 8 or 8 x 4");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  SampleRec* recs = reinterpret_cast<SampleRec*>(smem);
  __shared__ int lvlH[kMaxLevels], lvlW[kMaxLevels], lvlS[kMaxLevels];
  const int tid = threadIdx.x;
  if (tid < L) {
    lvlH[tid] = (int)shapes[2 * tid];
    lvlW[tid] = (int)shapes[2 * tid + 1];
    lvlS[tid] = (int)level_start[tid];
  }
  __syncthreads();
  const int MD = M * D;
  const int r = tid / G, j = tid % G;
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // flat (b, q); head = block % M (one head per XCD L2)
  const int m = blockIdx.x % M;
  const long long row = qrow * M + m;
  const bool live = qrow * M < rows;
  if (live) {      // whole row groups are live or not (G divides 64): the DPP / shuffle exchanges stay within live groups
    const int QW = 3 * M * NS;
    const float* qo = qproj + qrow * QW + m * NS * 2;
    const float* ql = qproj + qrow * QW + M * NS * 2 + m * NS;
    float x[U], mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      x[u] = ql[j + u * G];
      mx = fmaxf(mx, x[u]);
    }
    mx = row_max<G>(mx);
    float e[U], part = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = expf(x[u] - mx);
      part += e[u];
    }
    const float den = row_sum<G>(part);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int sidx = j + u * G, l = sidx / P;
      const float a = e[u] / den;
      const float2 off = *reinterpret_cast<const float2*>(qo + 2 * sidx);
      const float2 rf = *reinterpret_cast<const float2*>(ref + (qrow * L + l) * 2);
      const float lx = rf.x + off.x, ly = rf.y + off.y;
      *reinterpret_cast<float2*>(loc_out + (row * NS + sidx) * 2) = make_float2(lx, ly);
      attn_out[row * NS + sidx] = a;
      SampleRec rec;
      make_sample<float>(lx, ly, a, lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + sidx] = rec;
    }
  }
  __syncthreads();
  if (!live) return;
  const long long b = row / ((long long)Lq * M);
  const H* vbase = value + b * (long long)S * MD + m * D + CPL * j;
  float acc[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc[c] = 0.f;
  const SampleRec* rr = recs + r * NS;
  for (int s = 0; s < NS; ++s) {
    const SampleRec rec = rr[s];
    if (rec.mask == 0) continue;  // uniform across the row's lanes
    const float hy = 1.f - rec.ly, hx = 1.f - rec.lx;
    // all four corners loaded (an outside corner from the row's own first pixel), raw words masked, widened after the loads: as msda_fwd_h16
    const unsigned m1 = (rec.mask & 1) ? ~0u : 0u, m2 = (rec.mask & 2) ? ~0u : 0u, m3 = (rec.mask & 4) ? ~0u : 0u, m4 = (rec.mask & 8) ? ~0u : 0u;
    const int o1 = rec.off00 & (int)m1, o2 = (rec.off00 + MD) & (int)m2, o3 = (rec.off00 + rec.rowstride) & (int)m3,
              o4 = (rec.off00 + rec.rowstride + MD) & (int)m4;
    const auto r1 = ocpg_dev::keep(ldraw<CPL>(vbase + o1), m1), r2 = ocpg_dev::keep(ldraw<CPL>(vbase + o2), m2),
               r3 = ocpg_dev::keep(ldraw<CPL>(vbase + o3), m3), r4 = ocpg_dev::keep(ldraw<CPL>(vbase + o4), m4);
    float v1[CPL], v2[CPL], v3[CPL], v4[CPL];
    widen(r1, vbase, v1); widen(r2, vbase, v2); widen(r3, vbase, v3); widen(r4, vbase, v4);
    const float w1 = hy * hx, w2 = hy * rec.lx, w3 = rec.ly * hx, w4 = rec.ly * rec.lx;
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] += (w1 * v1[c] + w2 * v2[c] + w3 * v3[c] + w4 * v4[c]) * rec.a;
  }
  stc<CPL>(out + row * D + CPL * j, acc);
}

// Fused gather: msda_bwd_gather_h16 whose epilogue applies the backward of the module's softmax and writes the gradient of the merged query
// projection gq [N*Lq, 3*M*16] = [d offsets | d logits] instead of grad_loc / grad_attn.  Each sample's (d attn, d x, d y) totals stay
// in registers across the four batches: with G = 8 the lane pair p = j >> 1 holds the samples 4k + p (reduce_scatter_g8_p4, as the fp32
// kernel), with G = 4 lane j holds the samples 4k + j (reduce_scatter_g4_p4) and every lane stores.
template <typename H, int G, int CPL>
__global__ __launch_bounds__(256) void msda_bwd_gather_fused_h16(const H* __restrict__ value, const int64_t* __restrict__ shapes,
                                                                 const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                                 const float* __restrict__ attn, const H* __restrict__ gout, int S, int M,
                                                                 int L, int Lq, int P, long long rows, float* __restrict__ gq) {
  constexpr int D = CPL * G, ROWS = 256 / G, NS = 16, NB = 4;
  static_assert(D == 32 && (G == 4 || G == 8), "D = 32 as 4 x 8 or 8 x 4");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  GatherRec* recs = reinterpret_cast<GatherRec*>(smem);
  __shared__ int lvlH[kMaxLevels], lvlW[kMaxLevels], lvlS[kMaxLevels];
  const int tid = threadIdx.x;
  if (tid < L) {
    lvlH[tid] = (int)shapes[2 * tid];
    lvlW[tid] = (int)shapes[2 * tid + 1];
    lvlS[tid] = (int)level_start[tid];
  }
  __syncthreads();
  const int MD = M * D;
  const int r = tid / G, j = tid % G;
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // head fastest: one head per XCD L2
  const int m = blockIdx.x % M;
  const long long row = qrow * M + m;
  const bool live = qrow * M < rows;
  if (live) {
    const float* lrow = loc + row * NS * 2;
    const float* arow = attn + row * NS;
    for (int s = j; s < NS; s += G) {
      const int l = s / P;
      GatherRec rec;
      make_gather(lrow[2 * s], lrow[2 * s + 1], arow[s], lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + s] = rec;
    }
  }
  __syncthreads();
  if (!live) return;  // whole row groups leave together (G divides 64): the DPP exchanges below stay within live groups
  const long long b = row / ((long long)Lq * M);
  const H* vbase = value + b * (long long)S * MD + m * D + CPL * j;
  float go[CPL];
  ldc<CPL>(gout + row * D + CPL * j, go);
  const GatherRec* rr = recs + r * NS;
  float fga[4] = {0.f, 0.f, 0.f, 0.f}, fgx[4] = {0.f, 0.f, 0.f, 0.f}, fgy[4] = {0.f, 0.f, 0.f, 0.f};      // this lane's sample of each batch
  auto batch = [&](const int s0) {
    float red[NB][3];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const GatherRec rec = rr[s0 + i];
      const int bits = rec.pk & 15;
      const H* p00 = vbase + (rec.pk & ~15);
      const int dx = (bits & 3) == 3 ? MD : 0, dy = (bits & 12) == 12 ? rec.rowstride : 0;
      float v0[CPL], v1[CPL], v2[CPL], v3[CPL];
      ldc<CPL>(p00, v0); ldc<CPL>(p00 + dx, v1); ldc<CPL>(p00 + dy, v2); ldc<CPL>(p00 + dy + dx, v3);
      float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
      for (int c = 0; c < CPL; ++c) { d0 += go[c] * v0[c]; d1 += go[c] * v1[c]; d2 += go[c] * v2[c]; d3 += go[c] * v3[c]; }
      const float ix0 = (bits & 1) ? 1.f : 0.f, ix1 = (bits & 2) ? 1.f : 0.f, iy0 = (bits & 4) ? 1.f : 0.f, iy1 = (bits & 8) ? 1.f : 0.f;
      const float top = rec.hx * d0 + rec.lx * d1, bot = rec.hx * d2 + rec.lx * d3;          // rows ya / yb, x-interpolated
      const float lef = ix1 * d1 - ix0 * d0, rig = ix1 * d3 - ix0 * d2;                      // d/dx along rows ya / yb
      red[i][0] = rec.hy * top + rec.ly * bot;
      red[i][1] = rec.aW * (rec.hy * lef + rec.ly * rig);
      red[i][2] = rec.aH * (iy1 * bot - iy0 * top);
    }
    float tot[3];
    if constexpr (G == 8) (void)reduce_scatter_g8_p4(red, j, tot);
    else reduce_scatter_g4_p4(red, j, tot);
#pragma unroll
    for (int k = 0; k < 4; ++k) {       // (selects, not an indexed store: the batch loop stays rolled)
      const bool mine = s0 == NB * k;
      fga[k] = mine ? tot[0] : fga[k]; fgx[k] = mine ? tot[1] : fgx[k]; fgy[k] = mine ? tot[2] : fgy[k];
    }
  };
#pragma unroll 1
  for (int s0 = 0; s0 < NS; s0 += NB) batch(s0);
  // softmax backward over the row's 16 weights: d logit_s = a_s (ga_s - sum_t a_t ga_t)
  const int p = G == 8 ? j >> 1 : j;
  const bool owner = G == 4 || (j & 1) == 0;          // G = 8: both lanes of a pair hold the same totals, the even one counts and stores
  float av[4], dotp = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    av[k] = attn[row * NS + 4 * k + p];
    dotp += owner ? av[k] * fga[k] : 0.f;
  }
  const float dot = row_sum<G>(dotp);
  if (owner) {
    const int QW = 3 * M * NS;
    float* go_ = gq + qrow * QW + m * (NS * 2);
    float* gl_ = gq + qrow * QW + M * (NS * 2) + m * NS;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int sidx = 4 * k + p;
      *reinterpret_cast<float2*>(go_ + 2 * sidx) = make_float2(fgx[k], fgy[k]);
      gl_[sidx] = av[k] * (fga[k] - dot);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
inline int pow2_group(int D, int cpl) {
  if (D % cpl) return 0;
  const int g = D / cpl;
  if (g < 1 || g > 64 || (g & (g - 1))) return 0;
  return g;
}

inline int check_common(const void* a, const void* b, const void* c, const void* d, const void* e, int N, int S, int M, int D,
                        int L, int Lq, int P) {
  if (N < 0) return -1006;
  if (S <= 0) return -1007;
  if (M <= 0) return -1008;
  if (D <= 0) return -1009;
  if (L <= 0) return -1010;
  if (Lq < 0) return -1011;
  if (P <= 0) return -1012;
  if ((long long)N * Lq == 0) return 0;  // empty problem: pointers may legitimately be null
  if (!a) return -1001;
  if (!b) return -1002;
  if (!c) return -1003;
  if (!d) return -1004;
  if (!e) return -1005;
  return 0;
}

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// Channels per lane.  The compile-time defaults above are the decision; the variable exists for the A/B timing tool.  8 is a REQUEST:
// a shape whose records for 256 / G rows do not fit 48 KB of LDS (e.g. D = 16 with L * P = 16) is served with 4 channels per lane.
// OCPG_MSDA_H16_LANES=4|8 (read per call: the timing tool toggles it in-process) forces the channels per lane of the forward and gather
inline int lanes_cpl(int dflt) {
  const char* e = std::getenv("OCPG_MSDA_H16_LANES");
  if (e && e[0] == '4') return 4;
  if (e && e[0] == '8') return 8;
  return dflt;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what the fast kernels need beyond D: 32-bit element offsets, the level table, 16-byte aligned 16-bit buffers (rows of D >= 4
// elements then sit on the 8- / 16-byte boundaries the vector loads rely on).  Otherwise: the generic kernels.
inline bool fast_ok(int S, int M, int D, int L, const void* p0, const void* p1, const void* p2) {
  return L <= kMaxLevels && (long long)S * M * D < (1LL << 31) && aligned16(p0) && aligned16(p1) && aligned16(p2);
}

template <typename H>
int fwd_h16(const H* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn, int N, int S, int M,
            int D, int L, int Lq, int P, H* out, hipStream_t st) {
  const long long rows = (long long)N * Lq * M;
  const size_t rec_bytes = (size_t)L * P * sizeof(SampleRec);
  if (fast_ok(S, M, D, L, value, out, out)) {
    const int cpl = lanes_cpl(MSDA_H16_FWD_CPL);
    const int G8 = pow2_group(D, 8), G4 = pow2_group(D, 4);
#define FWD_LAUNCH(G_, CPL_)                                                                                                      \
  {                                                                                                                               \
    const int rpb = 256 / G_;                                                                                                     \
    const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);                                                  \
    msda_fwd_h16<H, G_, CPL_><<<grid, 256, rpb * rec_bytes, st>>>(value, shapes, level_start, loc, attn, S, M, L, Lq, P, rows, out); \
    return launch_status();                                                                                                       \
  }
    if (cpl == 8 && (G8 == 2 || G8 == 4 || G8 == 8) && (256 / G8) * rec_bytes <= 48 * 1024) {
      if (G8 == 2) FWD_LAUNCH(2, 8)
      if (G8 == 4) FWD_LAUNCH(4, 8)
      FWD_LAUNCH(8, 8)
    }
    if (G4 && (256 / G4) * rec_bytes <= 48 * 1024) {
      switch (G4) {
        case 1: FWD_LAUNCH(1, 4)
        case 2: FWD_LAUNCH(2, 4)
        case 4: FWD_LAUNCH(4, 4)
        case 8: FWD_LAUNCH(8, 4)
        case 16: FWD_LAUNCH(16, 4)
        case 32: FWD_LAUNCH(32, 4)
        default: FWD_LAUNCH(64, 4)
      }
    }
#undef FWD_LAUNCH
  }
  msda_fwd_generic_h16<H><<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(value, shapes, level_start, loc, attn, S, M, D, L, Lq, P, rows, out);
  return launch_status();
}

// the gather row kernel serves D in {16, 32}; 0 = not served (decided BEFORE anything is launched), else the channels per lane
inline int gather_cpl(int D, int L, int P) {
  if (D != 16 && D != 32) return 0;
  const int cpl = lanes_cpl(MSDA_H16_GATHER_CPL);
  const int G = D / cpl;
  return (256 / G) * (size_t)L * P * sizeof(GatherRec) <= 48 * 1024 ? cpl : 0;
}

template <typename H>
void launch_gather(int cpl, const H* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                   const H* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_loc, float* grad_attn, hipStream_t st) {
  const long long rows = (long long)N * Lq * M;
  const int G = D / cpl, rpb = 256 / G;
  const size_t glds = rpb * (size_t)L * P * sizeof(GatherRec);
  const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
#define GATHER_LAUNCH(G_, CPL_) \
  msda_bwd_gather_h16<H, G_, CPL_><<<grid, 256, glds, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, L, Lq, P, rows, grad_loc, grad_attn)
  if (cpl == 8) {
    if (G == 2) GATHER_LAUNCH(2, 8); else GATHER_LAUNCH(4, 8);
  } else {
    if (G == 4) GATHER_LAUNCH(4, 4); else GATHER_LAUNCH(8, 4);
  }
#undef GATHER_LAUNCH
}

template <typename H>
int bwd_h16(const H* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn, const H* grad_out,
            int N, int S, int M, int D, int L, int Lq, int P, float* grad_value, float* grad_loc, float* grad_attn,
            const int64_t* shapes_host, int* sel_state, int go_dtype, hipStream_t st) {
  const long long rows = (long long)N * Lq * M;
  // the single-level column scatter forced by OCPG_MSDA_COL_LP < 4 reads fp32 only: the whole backward takes the generic kernel then
  const bool legacy_forced = !ocpg_col::patch_kernel_allowed();
  const size_t rec_bytes = (size_t)L * P * sizeof(SampleRec);
  const int G = pow2_group(D, 4);
  if (!legacy_forced && G && (256 / G) * rec_bytes <= 48 * 1024 && fast_ok(S, M, D, L, value, grad_out, grad_out)) {
    // self-attention: grad_value through the column-scatter / output-tiled kernels (path selection included) + the gather row kernel;
    // the gather's conditions are settled first, so nothing has been launched when the pair is not served
    // (the output-tiled grad_value kernels want loc / attn / grad_value on 16 bytes too: settled here, so that no family can refuse after
    //  the other one has been launched)
    const int gcpl = gather_cpl(D, L, P);
    if (gcpl && shapes_host && Lq == S && aligned16(loc) && aligned16(attn) && aligned16(grad_value)) {
      const int rc = ocpg_msda::bwd_value_sel(loc, attn, grad_out, go_dtype, N, S, M, D, L, Lq, P, grad_value, shapes_host, sel_state, st);
      if (rc == 0) {
        launch_gather<H>(gcpl, value, shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Lq, P, grad_loc, grad_attn, st);
        return launch_status();
      }
      if (rc != -2000) return rc;
    }
    const int rpb = 256 / G;
    const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
    const size_t lds = rpb * rec_bytes;
#define ROW_LAUNCH(G_) \
  msda_bwd_row_h16<H, G_><<<grid, 256, lds, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, L, Lq, P, rows, grad_value, grad_loc, grad_attn); break
    switch (G) {
      case 1: ROW_LAUNCH(1);
      case 2: ROW_LAUNCH(2);
      case 4: ROW_LAUNCH(4);
      case 8: ROW_LAUNCH(8);
      case 16: ROW_LAUNCH(16);
      case 32: ROW_LAUNCH(32);
      default: ROW_LAUNCH(64);
    }
#undef ROW_LAUNCH
    return launch_status();
  }
  msda_bwd_generic_h16<H><<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, D, L, Lq, P, rows,
                                                                   grad_value, grad_loc, grad_attn);
  return launch_status();
}

// ---- fused front end: D = 32, L * P = 16 only; both lane mappings fit the LDS (64 rows x 16 records x 32 B = 32 KB with 8 channels per lane)
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

inline bool fused_shape_ok(int S, int M, int D, int L, int P) {
  return D == 32 && L * P == 16 && L <= kMaxLevels && (long long)S * M * D < (1LL << 31);
}

template <typename H>
void launch_fused_fwd(const H* value, const int64_t* shapes, const int64_t* level_start, const float* qproj, const float* ref, int N, int S,
                      int M, int L, int Lq, int P, H* out, float* loc_out, float* attn_out, hipStream_t st) {
  const long long rows = (long long)N * Lq * M;
  const int G = 32 / lanes_cpl(MSDA_H16_FWD_CPL), rpb = 256 / G;
  const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
  const size_t lds = rpb * (size_t)16 * sizeof(SampleRec);
  if (G == 4)
    msda_fwd_fused_h16<H, 4, 8><<<grid, 256, lds, st>>>(value, shapes, level_start, qproj, ref, S, M, L, Lq, P, rows, out, loc_out, attn_out);
  else
    msda_fwd_fused_h16<H, 8, 4><<<grid, 256, lds, st>>>(value, shapes, level_start, qproj, ref, S, M, L, Lq, P, rows, out, loc_out, attn_out);
}

template <typename H>
void launch_fused_gather(const H* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                         const H* grad_out, int N, int S, int M, int L, int Lq, int P, float* grad_qproj, hipStream_t st) {
  const long long rows = (long long)N * Lq * M;
  const int G = 32 / lanes_cpl(MSDA_H16_GATHER_CPL), rpb = 256 / G;
  const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
  const size_t lds = rpb * (size_t)16 * sizeof(GatherRec);
  if (G == 4)
    msda_bwd_gather_fused_h16<H, 4, 8><<<grid, 256, lds, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, L, Lq, P, rows, grad_qproj);
  else
    msda_bwd_gather_fused_h16<H, 8, 4><<<grid, 256, lds, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, L, Lq, P, rows, grad_qproj);
}

}  // namespace

extern "C" {

int ocpg_msda_fwd_h16(const void* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                      int N, int S, int M, int D, int L, int Lq, int P, void* out, const int64_t* shapes_host, int dtype, void* stream) {
  (void)shapes_host;      // accepted for symmetry with ocpg_msda_fwd_f32 (only its opt-in LDS-window forward reads it; no 16-bit version)
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  if (dtype != 1 && dtype != 2) return -1015;
  if ((long long)N * Lq * M == 0) return 0;
  if (!out) return -1013;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    return fwd_h16(static_cast<const bf16s*>(value), shapes, level_start, loc, attn, N, S, M, D, L, Lq, P, static_cast<bf16s*>(out), st);
  return fwd_h16(static_cast<const fp16s*>(value), shapes, level_start, loc, attn, N, S, M, D, L, Lq, P, static_cast<fp16s*>(out), st);
}

int ocpg_msda_bwd_h16(const void* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                      const void* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_value, float* grad_loc,
                      float* grad_attn, const int64_t* shapes_host, int* sel_state, int dtype, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  if (dtype != 1 && dtype != 2) return -1019;
  if ((long long)N * Lq * M == 0) return 0;
  if (!grad_out) return -1013;
  if (!grad_value) return -1014;
  if (!grad_loc) return -1015;
  if (!grad_attn) return -1016;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    return bwd_h16(static_cast<const bf16s*>(value), shapes, level_start, loc, attn, static_cast<const bf16s*>(grad_out), N, S, M, D, L, Lq,
                   P, grad_value, grad_loc, grad_attn, shapes_host, sel_state, dtype, st);
  return bwd_h16(static_cast<const fp16s*>(value), shapes, level_start, loc, attn, static_cast<const fp16s*>(grad_out), N, S, M, D, L, Lq, P,
                 grad_value, grad_loc, grad_attn, shapes_host, sel_state, dtype, st);
}

// The two halves of the self-attention backward on their own (include/ocpg_hip.h): -2000 = shape / forced path not served, nothing launched.
int ocpg_msda_bwd_value_h16(const float* loc, const float* attn, const void* grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                            float* grad_value, const int64_t* shapes_host, int* sel_state, int dtype, void* stream) {
  if (N < 0 || S <= 0 || M <= 0 || D <= 0 || L <= 0 || Lq < 0 || P <= 0) return -1006;
  if (dtype != 1 && dtype != 2) return -1014;
  if ((long long)N * Lq == 0) return 0;
  if (!loc) return -1001;
  if (!attn) return -1002;
  if (!grad_out) return -1003;
  if (!grad_value) return -1011;
  if (!aligned16(grad_out) || !aligned16(loc) || !aligned16(attn) || !aligned16(grad_value)) return -2000;     // before anything is launched
  if (int e = ocpg_msda::bwd_value_sel(loc, attn, grad_out, dtype, N, S, M, D, L, Lq, P, grad_value, shapes_host, sel_state, (hipStream_t)stream)) return e;
  return launch_status();
}

int ocpg_msda_bwd_locattn_h16(const void* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                              const void* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_loc, float* grad_attn,
                              int dtype, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  if (dtype != 1 && dtype != 2) return -1016;
  if ((long long)N * Lq * M == 0) return 0;
  if (!grad_out) return -1013;
  if (!grad_loc) return -1014;
  if (!grad_attn) return -1015;
  const int cpl = gather_cpl(D, L, P);
  if (!cpl || !fast_ok(S, M, D, L, value, grad_out, grad_out)) return -2000;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    launch_gather(cpl, static_cast<const bf16s*>(value), shapes, level_start, loc, attn, static_cast<const bf16s*>(grad_out), N, S, M, D, L, Lq, P,
                  grad_loc, grad_attn, st);
  else
    launch_gather(cpl, static_cast<const fp16s*>(value), shapes, level_start, loc, attn, static_cast<const fp16s*>(grad_out), N, S, M, D, L, Lq, P,
                  grad_loc, grad_attn, st);
  return launch_status();
}

// ---- fused front end (include/ocpg_hip.h): -2000 = shape or alignment not served, settled for every pointer before anything is launched ----
int ocpg_msda_fused_fwd_h16(const void* value, const int64_t* shapes, const int64_t* level_start, const float* qproj, const float* ref,
                            int N, int S, int M, int D, int L, int Lq, int P, void* out, float* loc_out, float* attn_out, int dtype,
                            void* stream) {
  if (int e = check_common(value, shapes, level_start, qproj, ref, N, S, M, D, L, Lq, P)) return e;
  if (dtype != 1 && dtype != 2) return -1016;
  if ((long long)N * Lq * M == 0) return 0;
  if (!out) return -1013;
  if (!loc_out) return -1014;
  if (!attn_out) return -1015;
  if (!fused_shape_ok(S, M, D, L, P)) return -2000;
  // 16-byte (8 channels) / 8-byte (4 channels) accesses to value and out: 16 asked of both mappings, as the un-fused kernels do; float2
  // accesses to the offsets, the reference points and loc_out
  if (!aligned16(value) || !aligned16(out) || !aligned8(qproj) || !aligned8(ref) || !aligned8(loc_out)) return -2000;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    launch_fused_fwd(static_cast<const bf16s*>(value), shapes, level_start, qproj, ref, N, S, M, L, Lq, P, static_cast<bf16s*>(out), loc_out,
                     attn_out, st);
  else
    launch_fused_fwd(static_cast<const fp16s*>(value), shapes, level_start, qproj, ref, N, S, M, L, Lq, P, static_cast<fp16s*>(out), loc_out,
                     attn_out, st);
  return launch_status();
}

int ocpg_msda_fused_bwd_qproj_h16(const void* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                                  const void* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_qproj, int dtype,
                                  void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  if (dtype != 1 && dtype != 2) return -1015;
  if ((long long)N * Lq * M == 0) return 0;
  if (!grad_out) return -1013;
  if (!grad_qproj) return -1014;
  if (!fused_shape_ok(S, M, D, L, P)) return -2000;
  if (!aligned16(value) || !aligned16(grad_out) || !aligned8(grad_qproj)) return -2000;       // (loc / attn are read one float at a time)
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1)
    launch_fused_gather(static_cast<const bf16s*>(value), shapes, level_start, loc, attn, static_cast<const bf16s*>(grad_out), N, S, M, L, Lq, P,
                        grad_qproj, st);
  else
    launch_fused_gather(static_cast<const fp16s*>(value), shapes, level_start, loc, attn, static_cast<const fp16s*>(grad_out), N, S, M, L, Lq, P,
                        grad_qproj, st);
  return launch_status();
}

}  // extern "C"
