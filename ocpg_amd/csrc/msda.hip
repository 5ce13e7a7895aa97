// MSDeformAttn forward / backward for MI355X (gfx950, wave64) -- hand-written HIP, no CUDA lineage.
//
// What it computes is fixed by the reference (models/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299 forward,
// :87-159 + :301-403 backward); how it is mapped onto the machine is not:
//
//   * a "row" is one (batch b, query q, head m); its D channels are contiguous (value is [N,S,M,D]).
//     The fast path gives a row G = D/4 lanes, each lane owning one float4 (16 B) of the head's channels, so
//     a corner fetch of a head is ONE 16-B-per-lane load covering the head's whole 4*D-byte line, and a
//     wave64 carries 64/G rows (D=32: one query x 8 heads = the query's full 1-KiB output line).
//   * the per-sample scalar work (pixel coords, bounds tests, bilinear weights, corner offsets) is done ONCE
//     per row by the row's lanes in parallel (lane j takes samples j, j+G, ...), parked in LDS, and then
//     re-read as wave-broadcast ds_read_b128 -- the reference redoes it in every one of the D channel
//     threads (32x redundant for D=32) together with int64 shape loads.
//   * backward: grad_loc / grad_attn need a sum over the row's D channels; that is a G-lane DPP-free
//     shuffle reduction in registers instead of the reference's shared-memory + thread-0 serial loop
//     (cuh:366-381).  grad_value is a float atomic scatter (one dword per lane per instruction).
//   * no im2col_step chunk loop on the host: one launch per call.
//
// The generic kernels (any D, float or double) keep one wave per row with lanes striding over channels;
// they exist for the reference's test protocol (models/ops/test.py:85: D in {30,71,1025,2048,3096}, fp64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "../../include/ocpg_hip.h"
#include "msda_col.h"
#include "msda_tile.h"
#include "msda_dev.h"
#include "msda_host.h"

namespace {

constexpr int kMaxLevels = 16;

using ocpg_dev::SampleRec;
using ocpg_dev::make_sample;
using ocpg_dev::GatherRec;
using ocpg_dev::make_gather;
using ocpg_dev::ld4;
using ocpg_dev::group_sum;
using ocpg_dev::reduce_scatter_g8_p4;

// ------------------------------------------------------------------------------------------------------
// Fast forward: D = 4*G, G in {1,2,4,8,16,32,64}.  256 threads = 256/G rows per block.
// LDS: rows_per_block * NS * 32 B (dynamic).
template <int G>
__global__ __launch_bounds__(256) void msda_fwd_fast(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                                                     const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                     const float* __restrict__ attn, int S, int M, int L, int Lq, int P,
                                                     long long rows, float* __restrict__ out) {
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
  // XCD-aware mapping: blocks are dealt round-robin over the 8 XCDs, so block % M picks the HEAD; with M == 8 every
  // XCD then gathers only its own head's 128-B slices of `value` (1/8 of the map) through its private 4-MiB L2.
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // flat (b, q)
  const long long row = qrow * M + (blockIdx.x % M);
  const bool live = qrow * M < rows;
  if (live) {
    const float* lrow = loc + row * NS * 2;
    const float* arow = attn + row * NS;
    for (int s = j; s < NS; s += G) {
      const int l = s / P;
      SampleRec rec;
      make_sample<float>(lrow[2 * s], lrow[2 * s + 1], arow[s], lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + s] = rec;
    }
  }
  __syncthreads();
  if (!live) return;
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const float* vbase = value + b * (long long)S * MD + m * D + 4 * j;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const SampleRec* rr = recs + r * NS;
  // (a 4-sample batched, branch-free variant of this loop measured SLOWER on MI355X: 84 vs 64 us at the encoder
  //  shape -- the gather is L1/TA-throughput bound, not latency bound, and the batch costs occupancy)
  int s = 0;
  for (; s < NS; ++s) {
    const SampleRec rec = rr[s];
    if (rec.mask == 0) continue;  // uniform across the row's lanes
    const float hy = 1.f - rec.ly, hx = 1.f - rec.lx;
    const float* p00 = vbase + rec.off00;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v1 = (rec.mask & 1) ? ld4(p00) : z;
    const float4 v2 = (rec.mask & 2) ? ld4(p00 + MD) : z;
    const float4 v3 = (rec.mask & 4) ? ld4(p00 + rec.rowstride) : z;
    const float4 v4 = (rec.mask & 8) ? ld4(p00 + rec.rowstride + MD) : z;
    const float w1 = hy * hx, w2 = hy * rec.lx, w3 = rec.ly * hx, w4 = rec.ly * rec.lx;
    acc.x += (w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x) * rec.a;
    acc.y += (w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y) * rec.a;
    acc.z += (w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z) * rec.a;
    acc.w += (w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w) * rec.a;
  }
  *reinterpret_cast<float4*>(out + row * D + 4 * j) = acc;
}

// ------------------------------------------------------------------------------------------------------
// Fused front end (round 4): the module's softmax over the L*P attention logits and `reference point + offset`
// (models/ops/modules/ms_deform_attn.py:96-110, the 2-d reference branch with the offsets already divided by (W_l, H_l) -- the
// caller folds that division into the projection's 256 weight rows) happen in the row's sample-setup phase, where the lanes compute
// per-sample scalars anyway.  Input: the merged query projection qproj [N*Lq, 3*M*NS] = [offsets (M, L, P, 2) | logits (M, L*P)] and
// ref [N*Lq, L, 2].  The sampling locations and attention weights are still WRITTEN (the backward kernels and the module's return
// value read them) but no longer produced by two elementwise passes and read back: -2 launches, -78 MB read per encoder layer at N = 10.
// D = 32 (G = 8), L*P = 16: lane j of a row owns samples j and j + 8.
__global__ __launch_bounds__(256) void msda_fwd_fused8(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ level_start, const float* __restrict__ qproj,
                                                       const float* __restrict__ ref, int S, int M, int L, int Lq, int P, long long rows,
                                                       float* __restrict__ out, float* __restrict__ loc_out, float* __restrict__ attn_out) {
  constexpr int G = 8, D = 32, ROWS = 256 / G, NS = 16;
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
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // flat (b, q); head = block % M (one head per XCD L2, see msda_fwd_fast)
  const int m = blockIdx.x % M;
  const long long row = qrow * M + m;
  const bool live = qrow * M < rows;
  if (live) {
    const int QW = 3 * M * NS;
    const float* qo = qproj + qrow * QW + m * NS * 2;
    const float* ql = qproj + qrow * QW + M * NS * 2 + m * NS;
    const float x0 = ql[j], x1 = ql[j + G];
    float mx = fmaxf(x0, x1);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float e0 = expf(x0 - mx), e1 = expf(x1 - mx);
    const float den = group_sum<G>(e0 + e1);
    const float a[2] = {e0 / den, e1 / den};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int sidx = j + u * G, l = sidx / P;
      const float2 off = *reinterpret_cast<const float2*>(qo + 2 * sidx);
      const float2 rf = *reinterpret_cast<const float2*>(ref + (qrow * L + l) * 2);
      const float lx = rf.x + off.x, ly = rf.y + off.y;
      *reinterpret_cast<float2*>(loc_out + (row * NS + sidx) * 2) = make_float2(lx, ly);
      attn_out[row * NS + sidx] = a[u];
      SampleRec rec;
      make_sample<float>(lx, ly, a[u], lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + sidx] = rec;
    }
  }
  __syncthreads();
  if (!live) return;
  const long long b = row / ((long long)Lq * M);
  const float* vbase = value + b * (long long)S * MD + m * D + 4 * j;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const SampleRec* rr = recs + r * NS;
  for (int sidx = 0; sidx < NS; ++sidx) {
    const SampleRec rec = rr[sidx];
    if (rec.mask == 0) continue;  // uniform across the row's lanes
    const float hy = 1.f - rec.ly, hx = 1.f - rec.lx;
    const float* p00 = vbase + rec.off00;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v1 = (rec.mask & 1) ? ld4(p00) : z;
    const float4 v2 = (rec.mask & 2) ? ld4(p00 + MD) : z;
    const float4 v3 = (rec.mask & 4) ? ld4(p00 + rec.rowstride) : z;
    const float4 v4 = (rec.mask & 8) ? ld4(p00 + rec.rowstride + MD) : z;
    const float w1 = hy * hx, w2 = hy * rec.lx, w3 = rec.ly * hx, w4 = rec.ly * rec.lx;
    acc.x += (w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x) * rec.a;
    acc.y += (w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y) * rec.a;
    acc.z += (w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z) * rec.a;
    acc.w += (w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w) * rec.a;
  }
  *reinterpret_cast<float4*>(out + row * D + 4 * j) = acc;
}

// ------------------------------------------------------------------------------------------------------
// Generic forward: one wave per row, lanes stride over channels.  Any D, float or double.
template <typename T>
__global__ __launch_bounds__(256) void msda_fwd_generic(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                                                        const int64_t* __restrict__ level_start, const T* __restrict__ loc,
                                                        const T* __restrict__ attn, int S, int M, int D, int L, int Lq, int P,
                                                        long long rows, T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int NS = L * P;
  const long long MD = (long long)M * D;
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const T* vb = value + b * (long long)S * MD + (long long)m * D;
  for (int c = lane; c < D; c += 64) {
    T acc = 0;
    for (int l = 0; l < L; ++l) {
      const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
      const long long ls = level_start[l];
      for (int p = 0; p < P; ++p) {
        const long long wi = row * NS + (long long)l * P + p;
        const T w_im = loc[2 * wi] * (T)W - (T)0.5, h_im = loc[2 * wi + 1] * (T)H - (T)0.5;
        if (!(h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W)) continue;
        const int y0 = (int)floor(h_im), x0 = (int)floor(w_im);
        const T ly = h_im - (T)y0, lx = w_im - (T)x0, hy = (T)1 - ly, hx = (T)1 - lx;
        const T* p00 = vb + (ls + (long long)y0 * W + x0) * MD + c;
        const bool y0ok = y0 >= 0, y1ok = y0 + 1 <= H - 1, x0ok = x0 >= 0, x1ok = x0 + 1 <= W - 1;
        const T v1 = (y0ok && x0ok) ? p00[0] : (T)0;
        const T v2 = (y0ok && x1ok) ? p00[MD] : (T)0;
        const T v3 = (y1ok && x0ok) ? p00[(long long)W * MD] : (T)0;
        const T v4 = (y1ok && x1ok) ? p00[(long long)W * MD + MD] : (T)0;
        acc += (hy * hx * v1 + hy * lx * v2 + ly * hx * v3 + ly * lx * v4) * attn[wi];
      }
    }
    out[row * D + c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------
// Gather side of the backward (grad_loc, grad_attn; cuh:87-159 without the col2im scatter): row kernel, used with the
// column-tile scatter kernel (msda_col.hip).  Differences from the gather in msda_bwd_fast<G>:
//   * validity is folded into the per-axis weights (hy' = y0 >= 0 ? 1-ly : 0 ...) and the corner addresses are clamped
//     into the map, so the inner loop has no masks and no selects: 4 unconditional 16-B loads, packed FMAs;
//   * 4 samples are reduced together by a DPP reduce-scatter (12 moves) instead of 9 LDS-crossbar shuffles per sample.

// FUSED (round 4; G = 8, L*P = 16): the epilogue applies the backward of the module's softmax and writes the gradient of the merged query
// projection [N*Lq, 3*M*NS] = [d offsets | d logits] (gloc = that matrix, gattn unused) instead of grad_loc / grad_attn -- ATen's
// softmax backward and the `cat` behind the split of the projection (78 MB copied per encoder layer at N = 10) disappear.
template <int G, bool FUSED = false>
__global__ __launch_bounds__(256) void msda_bwd_gather_row(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                                                           const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                           const float* __restrict__ attn, const float* __restrict__ gout, int S, int M,
                                                           int L, int Lq, int P, long long rows, float* __restrict__ gloc,
                                                           float* __restrict__ gattn) {
  constexpr int D = 4 * G;
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
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // head fastest: one head per XCD L2 (see msda_fwd_fast)
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
  const float* vbase = value + b * (long long)S * MD + m * D + 4 * j;
  const float4 go = ld4(gout + row * D + 4 * j);
  const GatherRec* rr = recs + r * NS;
  constexpr int NB = 4;
  float fga[4] = {0.f, 0.f, 0.f, 0.f}, fgx[4] = {0.f, 0.f, 0.f, 0.f}, fgy[4] = {0.f, 0.f, 0.f, 0.f};      // FUSED: this lane pair's sample of each batch
  auto batch = [&](const int s0) {
    float red[NB][3];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const bool have = s0 + i < NS;
      const GatherRec rec = rr[have ? s0 + i : s0];
      const int bits = rec.pk & 15;
      const float* p00 = vbase + (rec.pk & ~15);
      const int dx = (bits & 3) == 3 ? MD : 0, dy = (bits & 12) == 12 ? rec.rowstride : 0;
      const float4 v0 = ld4(p00), v1 = ld4(p00 + dx), v2 = ld4(p00 + dy), v3 = ld4(p00 + dy + dx);
      // per-corner dot products with the output gradient first: the weights then act on 4 scalars, not on 4 x D channels
      const float d0 = go.x * v0.x + go.y * v0.y + go.z * v0.z + go.w * v0.w;
      const float d1 = go.x * v1.x + go.y * v1.y + go.z * v1.z + go.w * v1.w;
      const float d2 = go.x * v2.x + go.y * v2.y + go.z * v2.z + go.w * v2.w;
      const float d3 = go.x * v3.x + go.y * v3.y + go.z * v3.z + go.w * v3.w;
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
    if (FUSED) {
      float tot[3];
      (void)reduce_scatter_g8_p4(red, j, tot);       // the lane pair j >> 1 now holds sample s0 + (j >> 1)
#pragma unroll
      for (int k = 0; k < 4; ++k) {       // (selects, not an indexed store: the batch loop stays rolled -- fully unrolled it took 256 registers)
        const bool mine = s0 == NB * k;
        fga[k] = mine ? tot[0] : fga[k]; fgx[k] = mine ? tot[1] : fgx[k]; fgy[k] = mine ? tot[2] : fgy[k];
      }
    } else if (G == 8 && s0 + NB <= NS) {
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
        const float ga = group_sum<G>(red[i][0]), gx = group_sum<G>(red[i][1]), gy = group_sum<G>(red[i][2]);
        if (j == 0) {
          const long long wi = row * NS + s0 + i;
          gattn[wi] = ga;
          *reinterpret_cast<float2*>(gloc + wi * 2) = make_float2(gx, gy);
        }
      }
    }
  };
#pragma unroll 1
  for (int s0 = 0; s0 < NS; s0 += NB) batch(s0);
  if (FUSED) {
    // softmax backward over the row's 16 weights: d logit_s = a_s (ga_s - sum_t a_t ga_t); the even lane of pair p holds samples 4k + p
    const int p = j >> 1;
    float av[4], dotp = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      av[k] = attn[row * 16 + 4 * k + p];
      dotp += (j & 1) ? 0.f : av[k] * fga[k];
    }
    const float dot = group_sum<G>(dotp);
    if ((j & 1) == 0) {
      const int QW = 3 * M * 16;
      float* go_ = gloc + qrow * QW + (row - qrow * M) * 32;
      float* gl_ = gloc + qrow * QW + M * 32 + (row - qrow * M) * 16;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sidx = 4 * k + p;
        *reinterpret_cast<float2*>(go_ + 2 * sidx) = make_float2(fgx[k], fgy[k]);
        gl_[sidx] = av[k] * (fga[k] - dot);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// Fast backward (plain float-atomic scatter for grad_value).
template <int G>
__global__ __launch_bounds__(256) void msda_bwd_fast(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                                                     const int64_t* __restrict__ level_start, const float* __restrict__ loc,
                                                     const float* __restrict__ attn, const float* __restrict__ gout, int S, int M,
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
  const long long qrow = (long long)(blockIdx.x / M) * ROWS + r;          // head fastest: one head per XCD L2 (see msda_fwd_fast)
  const long long row = qrow * M + (blockIdx.x % M);
  const bool live = qrow * M < rows;
  if (live) {
    const float* lrow = loc + row * NS * 2;
    const float* arow = attn + row * NS;
    for (int s = j; s < NS; s += G) {
      const int l = s / P;
      SampleRec rec;
      make_sample<float>(lrow[2 * s], lrow[2 * s + 1], arow[s], lvlH[l], lvlW[l], lvlS[l], MD, rec);
      recs[r * NS + s] = rec;
    }
  }
  __syncthreads();
  if (!live) return;  // whole row groups leave together (G divides 64): shuffles below stay within live groups
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const long long boff = b * (long long)S * MD + m * D + 4 * j;
  const float* vbase = value + boff;
  float* gsc = gvalue + b * (long long)S * MD + m * D + j;
  const float4 go = ld4(gout + row * D + 4 * j);
  const float gs[4] = {gout[row * D + j], gout[row * D + j + G], gout[row * D + j + 2 * G], gout[row * D + j + 3 * G]};
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
          float* g = gsc + rec.off00 + offs[k];        // lane j owns channels {j, j+G, j+2G, j+3G}: contiguous 4G-byte segments
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

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Generic backward: one wave per row; any D; float or double.
template <typename T>
__global__ __launch_bounds__(256) void msda_bwd_generic(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                                                        const int64_t* __restrict__ level_start, const T* __restrict__ loc,
                                                        const T* __restrict__ attn, const T* __restrict__ gout, int S, int M, int D,
                                                        int L, int Lq, int P, long long rows, T* __restrict__ gvalue,
                                                        T* __restrict__ gloc, T* __restrict__ gattn) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int NS = L * P;
  const long long MD = (long long)M * D;
  const int m = (int)(row % M);
  const long long b = row / ((long long)Lq * M);
  const long long boff = b * (long long)S * MD + (long long)m * D;
  for (int l = 0; l < L; ++l) {
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    const long long ls = level_start[l];
    for (int p = 0; p < P; ++p) {
      const long long wi = row * NS + (long long)l * P + p;
      const T w_im = loc[2 * wi] * (T)W - (T)0.5, h_im = loc[2 * wi + 1] * (T)H - (T)0.5;
      T ga = 0, gx = 0, gy = 0;
      if (h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W) {
        const int y0 = (int)floor(h_im), x0 = (int)floor(w_im);
        const T ly = h_im - (T)y0, lx = w_im - (T)x0, hy = (T)1 - ly, hx = (T)1 - lx;
        const T a = attn[wi];
        const bool ok[4] = {y0 >= 0 && x0 >= 0, y0 >= 0 && x0 + 1 <= W - 1, y0 + 1 <= H - 1 && x0 >= 0,
                            y0 + 1 <= H - 1 && x0 + 1 <= W - 1};
        const T w[4] = {hy * hx, hy * lx, ly * hx, ly * lx};
        const T dyc[4] = {-hx, -lx, hx, lx};
        const T dxc[4] = {-hy, hy, -ly, ly};
        const long long o00 = boff + (ls + (long long)y0 * W + x0) * MD;
        const long long offs[4] = {0, MD, (long long)W * MD, (long long)W * MD + MD};
        for (int c = lane; c < D; c += 64) {
          const T tg = gout[row * D + c];
          const T tga = tg * a;
          T val = 0, dx = 0, dy = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (ok[k]) {
              const T v = value[o00 + offs[k] + c];
              atomicAdd(gvalue + o00 + offs[k] + c, w[k] * tga);
              val += w[k] * v;
              dx += dxc[k] * v;
              dy += dyc[k] * v;
            }
          }
          ga += tg * val;
          gx += (T)W * dx * tga;
          gy += (T)H * dy * tga;
        }
      }
      ga = wave_sum<T>(ga);
      gx = wave_sum<T>(gx);
      gy = wave_sum<T>(gy);
      if (lane == 0) {
        gattn[wi] = ga;
        gloc[2 * wi] = gx;
        gloc[2 * wi + 1] = gy;
      }
    }
  }
}

inline int fast_group(int D) {
  if (D % 4) return 0;
  const int g = D / 4;
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

// OCPG_MSDA_COL=0 keeps the row kernel with its atomic scatter for every shape (A/B timing and parity); default: column kernels
inline bool col_enabled() {
  const char* e = std::getenv("OCPG_MSDA_COL");      // read per call: tests toggle it in-process
  return !(e && e[0] == '0');
}

// The column-tile FORWARD (LDS-staged value windows) is correct but, at config #2, slower than the row kernel
// (185 vs 100 us: DESIGN.md section 4.1): opt-in with OCPG_MSDA_FWD=col.
inline bool col_fwd_enabled() {
  const char* e = std::getenv("OCPG_MSDA_FWD");
  return col_enabled() && e && e[0] == 'c';
}

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// The column scatter's geometry: 8 x 16 query tiles on the finest level, LDS window margins kScatterMarginLo / kMarginHi (msda_col.h).
inline bool scatter_col_geom(const int64_t* shapes_host, int L, int S, int M, int P, ocpg_col::ColGeom& cg) {
  return ocpg_col::make_col_geom(shapes_host, L, S, M, P, 8, 16, cg, ocpg_col::kScatterMarginLo, ocpg_col::kMarginHi);
}

// ---- the two halves of the self-attention backward (also exported on their own: include/ocpg_hip.h) -----------------
// 1 = launched, 0 = shape not served by these kernels
// go_dtype: storage of grad_out (0 = float32, 1 = bfloat16, 2 = float16: the _h16 entry points of msda_h16.hip)
inline int launch_bwd_value_col(const float* loc, const float* attn, const void* grad_out, const int64_t* shapes_host, int N, int S,
                                int M, int D, int L, int Lq, int P, float* grad_value, hipStream_t st, int go_dtype = 0) {
  const int G = fast_group(D);
  if (!(shapes_host && Lq == S && col_enabled() && (G == 4 || G == 8) && (long long)S * M * D < (1LL << 31))) return 0;
  // round 3: output-tiled kernels (plain stores for the fine levels, no halo re-flush: csrc/msda_tile.hip).  Measured at config #2,
  // N = 10 (tools/bench_msda_gv.py, profiles/r03_msda_gv_paths.json): 261-280 us against the column scatter's 213 us on the model's
  // INITIAL ring offsets, 334-364 against 502 us on perturbed ("trained") offsets -- opt-in (OCPG_MSDA_TILE=1) until it wins both.
  const char* te = std::getenv("OCPG_MSDA_TILE");
  if (te && te[0] == '1' && ocpg_tile::bwd_value_tile(loc, attn, grad_out, shapes_host, N, S, M, D, L, P, grad_value, st, nullptr, 0, go_dtype)) return 1;
  ocpg_col::ColGeom cg;
  if (!scatter_col_geom(shapes_host, L, S, M, P, cg)) return 0;
  return ocpg_col::bwd_scatter_col(loc, attn, grad_out, N, S, M, D, P, cg, grad_value, st, nullptr, 0, go_dtype);
}

inline int launch_bwd_locattn_row(const float* value, const int64_t* shapes, const int64_t* level_start, const float* loc,
                                  const float* attn, const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                                  float* grad_loc, float* grad_attn, hipStream_t st) {
  const int G = fast_group(D);
  if (!((G == 4 || G == 8) && L <= kMaxLevels && (long long)S * M * D < (1LL << 31))) return 0;
  const int rpb = 256 / G;
  const size_t glds = rpb * (size_t)L * P * sizeof(GatherRec);
  if (glds > 48 * 1024) return 0;
  const long long rows = (long long)N * Lq * M;
  const unsigned ggrid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
  if (G == 4) msda_bwd_gather_row<4><<<ggrid, 256, glds, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, L, Lq, P, rows, grad_loc, grad_attn);
  else msda_bwd_gather_row<8><<<ggrid, 256, glds, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, L, Lq, P, rows, grad_loc, grad_attn);
  return 1;
}

}  // namespace

// grad_value of the self-attention shape for every grad_out storage type (msda_host.h): the body of ocpg_msda_bwd_value_sel_f32.
// 0 = launched, -2000 = shape / forced path not served (nothing launched), -2001 / -2002 = a family refused after the geometry checks.
int ocpg_msda::bwd_value_sel(const float* loc, const float* attn, const void* grad_out, int go_dtype, int N, int S, int M, int D, int L,
                             int Lq, int P, float* grad_value, const int64_t* shapes_host, int* sel_state, hipStream_t st) {
  const bool forced = std::getenv("OCPG_MSDA_TILE") != nullptr || !col_enabled();
  if (sel_state && !forced && shapes_host && Lq == S && D == 32 && (long long)S * M * D < (1LL << 31)) {
    // thresholds (percent of far samples as the ACTIVE family counts them), measured at config #2, N = 10 (tools/bench_msda_gv.py, GV_SELECT=1):
    //   offsets                      column: far share, us      tiled: far share, us
    //   initial ring                      0.0 %   169                0.0 %   279
    //   ring + N(0, 1.5 px) + 2 % far     3.0 %   241                3.6 %   305
    //   ring + N(0, 3 px) + 5 % far       9.3 %   432               12.5 %   361
    static const int to_tile = [] { const char* e = std::getenv("OCPG_MSDA_SEL_TO_TILE"); return e ? std::atoi(e) : 6; }();
    static const int to_col = [] { const char* e = std::getenv("OCPG_MSDA_SEL_TO_COL"); return e ? std::atoi(e) : 6; }();
    ocpg_col::ColGeom cg;
    if (scatter_col_geom(shapes_host, L, S, M, P, cg) && ocpg_col::select_supported(cg, D, P) &&
        ocpg_tile::tile_supported(shapes_host, N, L, S, M, P, D)) {
      if (ocpg_col::bwd_scatter_col(loc, attn, grad_out, N, S, M, D, P, cg, grad_value, st, sel_state, to_tile, go_dtype) != 2) return -2001;
      if (!ocpg_tile::bwd_value_tile(loc, attn, grad_out, shapes_host, N, S, M, D, L, P, grad_value, st, sel_state, to_col, go_dtype)) return -2002;
      ocpg_col::select_commit(sel_state, to_tile, to_col, st);
      return 0;
    }
  }
  if (!launch_bwd_value_col(loc, attn, grad_out, shapes_host, N, S, M, D, L, Lq, P, grad_value, st, go_dtype)) return -2000;
  return 0;
}


#define FAST_DISPATCH(G_, KERNEL, ...)                                                          \
  switch (G_) {                                                                                 \
    case 1: KERNEL<1><<<grid, 256, lds, st>>>(__VA_ARGS__); break;                               \
    case 2: KERNEL<2><<<grid, 256, lds, st>>>(__VA_ARGS__); break;                               \
    case 4: KERNEL<4><<<grid, 256, lds, st>>>(__VA_ARGS__); break;                               \
    case 8: KERNEL<8><<<grid, 256, lds, st>>>(__VA_ARGS__); break;                               \
    case 16: KERNEL<16><<<grid, 256, lds, st>>>(__VA_ARGS__); break;                             \
    case 32: KERNEL<32><<<grid, 256, lds, st>>>(__VA_ARGS__); break;                             \
    default: KERNEL<64><<<grid, 256, lds, st>>>(__VA_ARGS__); break;                             \
  }

extern "C" {

const char* ocpg_hip_version(void) { return "ocpg_hip gfx950 r4"; }

int ocpg_msda_fwd_f32(const float* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                      int N, int S, int M, int D, int L, int Lq, int P, float* out, const int64_t* shapes_host, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!out) return -1013;
  hipStream_t st = (hipStream_t)stream;
  const int G = fast_group(D);
  if (shapes_host && Lq == S && col_fwd_enabled() && (long long)S * M * D < (1LL << 31)) {
    ocpg_col::ColGeom cg;
    if (ocpg_col::make_col_geom(shapes_host, L, S, M, P, 8, 8, cg) && ocpg_col::fwd_col(value, loc, attn, N, S, M, D, P, cg, out, st))
      return launch_status();
  }
  const size_t rec_bytes = (size_t)L * P * sizeof(SampleRec);
  if (G && L <= kMaxLevels && (256 / G) * rec_bytes <= 48 * 1024 && (long long)S * M * D < (1LL << 31)) {
    const int rpb = 256 / G;
    const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
    const size_t lds = rpb * rec_bytes;
    // (a mask-free variant with validity folded into the weights, as in msda_bwd_gather_row, measured 109 vs 100 us: the
    //  forward is bound by the 16-B-per-lane gather path, not by its selects)
    FAST_DISPATCH(G, msda_fwd_fast, value, shapes, level_start, loc, attn, S, M, L, Lq, P, rows, out)
  } else {
    const unsigned grid = (unsigned)((rows + 3) / 4);
    msda_fwd_generic<float><<<grid, 256, 0, st>>>(value, shapes, level_start, loc, attn, S, M, D, L, Lq, P, rows, out);
  }
  return launch_status();
}

int ocpg_msda_fwd_f64(const double* value, const int64_t* shapes, const int64_t* level_start, const double* loc,
                      const double* attn, int N, int S, int M, int D, int L, int Lq, int P, double* out, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!out) return -1013;
  const unsigned grid = (unsigned)((rows + 3) / 4);
  msda_fwd_generic<double><<<grid, 256, 0, (hipStream_t)stream>>>(value, shapes, level_start, loc, attn, S, M, D, L, Lq, P, rows, out);
  return launch_status();
}

int ocpg_msda_bwd_f32(const float* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                      const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_value, float* grad_loc,
                      float* grad_attn, const int64_t* shapes_host, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!grad_out) return -1013;
  if (!grad_value) return -1014;
  if (!grad_loc) return -1015;
  if (!grad_attn) return -1016;
  hipStream_t st = (hipStream_t)stream;
  const int G = fast_group(D);
  const size_t rec_bytes = (size_t)L * P * sizeof(SampleRec);
  if (G && L <= kMaxLevels && (256 / G) * rec_bytes <= 48 * 1024 && (long long)S * M * D < (1LL << 31)) {
    const int rpb = 256 / G;
    // Self-attention backward = two independent kernels: the column-tile scatter (grad_value; reads loc / attn / grad_out)
    // and the row gather (grad_loc, grad_attn; reads value too).  (Running them on two streams was measured: 405 vs
    // 415 us -- each fills the chip on its own -- so both stay on the caller's stream.)
    if (launch_bwd_value_col(loc, attn, grad_out, shapes_host, N, S, M, D, L, Lq, P, grad_value, st)) {
      // the scatter takes G in {4, 8} only and the two row kernels' LDS records have one size, so the gather takes whatever the
      // enclosing condition took; a refusal here would be a bug, reported like a family that refuses after the geometry checks
      static_assert(sizeof(GatherRec) == sizeof(SampleRec), "launch_bwd_locattn_row must accept what the fast-path condition accepted");
      if (!launch_bwd_locattn_row(value, shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Lq, P, grad_loc, grad_attn, st)) return -2001;
      return launch_status();
    }
    const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
    const size_t lds = rpb * rec_bytes;
    FAST_DISPATCH(G, msda_bwd_fast, value, shapes, level_start, loc, attn, grad_out, S, M, L, Lq, P, rows, grad_value, grad_loc,
                  grad_attn)
  } else {
    const unsigned grid = (unsigned)((rows + 3) / 4);
    msda_bwd_generic<float><<<grid, 256, 0, st>>>(value, shapes, level_start, loc, attn, grad_out, S, M, D, L, Lq, P, rows,
                                                  grad_value, grad_loc, grad_attn);
  }
  return launch_status();
}

int ocpg_msda_bwd_value_f32(const float* loc, const float* attn, const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                            float* grad_value, const int64_t* shapes_host, void* stream) {
  return ocpg_msda_bwd_value_sel_f32(loc, attn, grad_out, N, S, M, D, L, Lq, P, grad_value, shapes_host, nullptr, stream);
}

// grad_value with per-call path selection (include/ocpg_hip.h).  Both paths' kernels are launched; the call site's state decides on the
// device which of them runs (csrc/msda_col.h).  Shapes, or forced paths (OCPG_MSDA_TILE / OCPG_MSDA_COL / OCPG_MSDA_COL_LP < 4), that do not
// allow the choice take the plain entry point's route and leave the state untouched.
int ocpg_msda_bwd_value_sel_f32(const float* loc, const float* attn, const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                                float* grad_value, const int64_t* shapes_host, int* sel_state, void* stream) {
  if (N < 0 || S <= 0 || M <= 0 || D <= 0 || L <= 0 || Lq < 0 || P <= 0) return -1006;
  if ((long long)N * Lq == 0) return 0;
  if (!loc) return -1001;
  if (!attn) return -1002;
  if (!grad_out) return -1003;
  if (!grad_value) return -1011;
  if (int e = ocpg_msda::bwd_value_sel(loc, attn, grad_out, 0, N, S, M, D, L, Lq, P, grad_value, shapes_host, sel_state, (hipStream_t)stream)) return e;
  return launch_status();
}

// ---- fused front end (include/ocpg_hip.h): D = 32, L * P = 16; anything else returns -2000 (the caller keeps the unfused path) ----------
int ocpg_msda_fused_fwd_f32(const float* value, const int64_t* shapes, const int64_t* level_start, const float* qproj, const float* ref,
                            int N, int S, int M, int D, int L, int Lq, int P, float* out, float* loc_out, float* attn_out, void* stream) {
  if (int e = check_common(value, shapes, level_start, qproj, ref, N, S, M, D, L, Lq, P)) return e;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!out) return -1013;
  if (!loc_out) return -1014;
  if (!attn_out) return -1015;
  if (D != 32 || L * P != 16 || L > kMaxLevels || (long long)S * M * D >= (1LL << 31)) return -2000;
  const int rpb = 256 / 8;
  const unsigned grid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
  msda_fwd_fused8<<<grid, 256, rpb * 16 * sizeof(SampleRec), (hipStream_t)stream>>>(value, shapes, level_start, qproj, ref, S, M, L, Lq, P, rows, out,
                                                                                   loc_out, attn_out);
  return launch_status();
}

int ocpg_msda_fused_bwd_qproj_f32(const float* value, const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                                  const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_qproj, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!grad_out) return -1013;
  if (!grad_qproj) return -1014;
  if (D != 32 || L * P != 16 || L > kMaxLevels || (long long)S * M * D >= (1LL << 31)) return -2000;
  const int rpb = 256 / 8;
  const unsigned ggrid = (unsigned)((((long long)N * Lq + rpb - 1) / rpb) * M);
  msda_bwd_gather_row<8, true><<<ggrid, 256, rpb * (size_t)16 * sizeof(GatherRec), (hipStream_t)stream>>>(value, shapes, level_start, loc, attn, grad_out, S, M, L,
                                                                                                      Lq, P, rows, grad_qproj, nullptr);
  return launch_status();
}

int ocpg_msda_bwd_locattn_f32(const float* value, const int64_t* shapes, const int64_t* level_start, const float* loc,
                              const float* attn, const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                              float* grad_loc, float* grad_attn, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  if ((long long)N * Lq * M == 0) return 0;
  if (!grad_out) return -1013;
  if (!grad_loc) return -1014;
  if (!grad_attn) return -1015;
  if (!launch_bwd_locattn_row(value, shapes, level_start, loc, attn, grad_out, N, S, M, D, L, Lq, P, grad_loc, grad_attn, (hipStream_t)stream))
    return -2000;
  return launch_status();
}

int ocpg_msda_bwd_f64(const double* value, const int64_t* shapes, const int64_t* level_start, const double* loc,
                      const double* attn, const double* grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                      double* grad_value, double* grad_loc, double* grad_attn, void* stream) {
  if (int e = check_common(value, shapes, level_start, loc, attn, N, S, M, D, L, Lq, P)) return e;
  const long long rows = (long long)N * Lq * M;
  if (rows == 0) return 0;
  if (!grad_out) return -1013;
  if (!grad_value) return -1014;
  if (!grad_loc) return -1015;
  if (!grad_attn) return -1016;
  const unsigned grid = (unsigned)((rows + 3) / 4);
  msda_bwd_generic<double><<<grid, 256, 0, (hipStream_t)stream>>>(value, shapes, level_start, loc, attn, grad_out, S, M, D, L,
                                                                   Lq, P, rows, grad_value, grad_loc, grad_attn);
  return launch_status();
}

}  // extern "C"
