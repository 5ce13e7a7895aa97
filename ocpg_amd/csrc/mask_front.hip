// Mask-head front end: the memory fusion  fusion = x_0 + R_1 x_1 + R_2 x_2  read straight from the encoder output and written in the
// two layouts its consumers want, and its backward, one launch each way.  (Second half of the file: the level-set feature stack.)
//
// The torch composition it stands for (models/ocpg.py, models/deformable_transformer.py): three slice + permute + contiguous copies of
// the token-major memory [N, S, C], two broadcast matmuls per coarser level (resample.bicubic_resize), two adds, and the channels-last
// copy ls_feat_viz's kernel reads; backward four more matmuls, the copies again, a zeros + copy + add per slice and a strided add of the
// two consumers' gradients.
//
// Geometry: level l is an [h_l, w_l, C] channels-last block at token start_l of every frame.  R_l = My_l (x) Mx_l with the dense 1-D
// matrices My_l [h_0, h_l], Mx_l [w_0, w_l] the host built (resample.bicubic_matrix: these are the operands of today's matmuls, bit for
// bit) and, per output index and per source index, the range (first, count) of the matrix entries that are not zero.  The kernels walk
// those ranges and read the weights from the matrices; they assume nothing about the ratio of the sizes (served: h_l <= h_0, w_l <= w_0).
// Every range read from device memory is clamped into its axis before it addresses anything.
//
// Thread shape, both kernels: 256 threads = 16 pixel slots x 16 lanes, a lane owns 4 consecutive channels of a 64-channel slab, so a
// global access of the token-major side is a float4 and the 16 lanes of a slot cover 256 consecutive bytes of one token.
//
// Forward, workgroup = (output row y, slab, frame):
//   1. vertical pass into LDS: v_l[j][c] = sum_i My_l[y, i] * x_l[i, j, c] for every column j of every coarser level;
//   2. per output column x: x_0[y, x, c] + sum_l sum_j Mx_l[x, j] * v_l[j][c]; the float4 goes to the channels-last port as it is and
//      into an LDS tile [64][stride] (stride % 16 == 1: the 16 lanes x 4 columns of a wave hit 64 different banks) from which the NCHW
//      port is written in runs along x.
// Backward, workgroup = (row i of level l, slab, frame), gather form, no atomics:
//   A. u[x][c] = sum_y My_l[y, i] * (g_nchw[c, y, x] + g_cl[y, x, c]) over the fine rows y whose matrix entry is not zero, into LDS
//      [w_0][68]; the NCHW gradient is read in runs along x by a 16 x-columns x 4 channels wave shape (bank = 4 x + c: no conflict),
//      the channels-last one by the float4 shape, each port only when it is there;
//   B. g_mem[l][i, j, c] = sum_x Mx_l[x, j] * u[x][c] over the fine columns of source column j.
//   Level 0 is the identity (one row, weight 1, copy); the rows of the levels that were not read are written as zeros.
// The gather loops issue their global loads four at a time (a tap past the end of a range re-reads the range's last row with weight 0,
// which adds an exact zero): one load in flight per thread left the backward latency-bound.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int NT = 256;
constexpr int SLAB = 64;           // channels per workgroup
constexpr int QL = SLAB / 4;       // lanes per pixel slot
constexpr int SLOTS = NT / QL;     // pixel slots
constexpr int MAXL = 6;            // levels in a memory
constexpr int USTR = SLAB + 4;     // row stride of the backward's u tile (floats): keeps float4 alignment, spreads the transposing stores
constexpr int MAX_LDS = 65536;
constexpr int UNR = 4;             // independent global loads per thread in the gather loops

struct Geo {
  int total, used;                 // levels in the memory, levels read
  int h[MAXL], w[MAXL], start[MAXL];
  int wy[MAXL], wx[MAXL];          // float offsets of My_l, Mx_l in wts
  int fy[MAXL], fx[MAXL];          // int offsets in rng: forward ranges per output row / column: (first source index, count)
  int by[MAXL], bx[MAXL];          // backward ranges per source row / column: (first output index, count)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void range(const int* __restrict__ rng, int off, int idx, int n, int& lo, int& cnt) {
  lo = clampi(rng[off + 2 * idx], 0, n - 1);
  cnt = clampi(rng[off + 2 * idx + 1], 0, n - lo);
}

__device__ __forceinline__ void fma4(float4& a, float s, const float4& v) {
  a.x += s * v.x; a.y += s * v.y; a.z += s * v.z; a.w += s * v.w;
}

__global__ __launch_bounds__(NT) void k_memfuse_fwd(const float* __restrict__ mem, const float* __restrict__ wts, const int* __restrict__ rng,
                                                    Geo g, int S, int C, int tstr, float* __restrict__ out_nchw,
                                                    float* __restrict__ out_cl) {
  extern __shared__ __align__(16) float lds[];
  const int y = blockIdx.x, c0 = blockIdx.y * SLAB, n = blockIdx.z;
  const int q = threadIdx.x & (QL - 1), slot = threadIdx.x / QL;
  const int c = c0 + 4 * q;
  const bool cok = c < C;
  const int h0 = g.h[0], w0 = g.w[0];
  const float* mb = mem + (size_t)n * S * C;

  // ---- 1: vertical pass of the coarser levels
  int voff = 0;
  for (int l = 1; l < g.used; ++l) {
    const int hl = g.h[l], wl = g.w[l];
    int lo, cnt;
    range(rng, g.fy[l], y, hl, lo, cnt);
    const float* my = wts + g.wy[l] + (size_t)y * hl;
    const float* src = mb + (size_t)g.start[l] * C + c;
    for (int j = slot; j < wl; j += SLOTS) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cok)
        for (int k0 = 0; k0 < cnt; k0 += UNR) {           // UNR loads in flight; a tap past the range re-reads the last row with weight 0
          float wv[UNR];
          float4 v[UNR];
#pragma unroll
          for (int t = 0; t < UNR; ++t) {
            const int k = k0 + t < cnt ? k0 + t : cnt - 1;
            wv[t] = k0 + t < cnt ? my[lo + k] : 0.f;
            v[t] = *reinterpret_cast<const float4*>(src + (size_t)((lo + k) * wl + j) * C);
          }
#pragma unroll
          for (int t = 0; t < UNR; ++t) fma4(acc, wv[t], v[t]);
        }
      *reinterpret_cast<float4*>(lds + voff + j * SLAB + 4 * q) = acc;
    }
    voff += wl * SLAB;
  }
  __syncthreads();

  // ---- 2: horizontal pass + level 0
  float* tile = lds + voff;
  for (int x = slot; x < w0; x += SLOTS) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok) acc = *reinterpret_cast<const float4*>(mb + (size_t)(g.start[0] + y * w0 + x) * C + c);
    int vo = 0;
    for (int l = 1; l < g.used; ++l) {
      const int wl = g.w[l];
      int lo, cnt;
      range(rng, g.fx[l], x, wl, lo, cnt);
      const float* mx = wts + g.wx[l] + (size_t)x * wl;
      for (int k = 0; k < cnt; ++k)
        fma4(acc, mx[lo + k], *reinterpret_cast<const float4*>(lds + vo + (lo + k) * SLAB + 4 * q));
      vo += wl * SLAB;
    }
    if (out_cl != nullptr && cok)
      *reinterpret_cast<float4*>(out_cl + ((size_t)(n * h0 + y) * w0 + x) * C + c) = acc;
    if (out_nchw != nullptr) {
      tile[(4 * q + 0) * tstr + x] = acc.x;
      tile[(4 * q + 1) * tstr + x] = acc.y;
      tile[(4 * q + 2) * tstr + x] = acc.z;
      tile[(4 * q + 3) * tstr + x] = acc.w;
    }
  }
  if (out_nchw != nullptr) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < SLAB * w0; idx += NT) {
      const int cc = idx / w0, x = idx - cc * w0;
      if (c0 + cc < C) out_nchw[((size_t)(n * C + c0 + cc) * h0 + y) * w0 + x] = tile[cc * tstr + x];
    }
  }
}

__global__ __launch_bounds__(NT) void k_memfuse_bwd(const float* __restrict__ g_nchw, const float* __restrict__ g_cl,
                                                    const float* __restrict__ wts, const int* __restrict__ rng, Geo g, int S, int C,
                                                    float* __restrict__ g_mem) {
  extern __shared__ __align__(16) float u[];               // [w0][USTR]
  const int c0 = blockIdx.y * SLAB, n = blockIdx.z;
  const int q = threadIdx.x & (QL - 1), slot = threadIdx.x / QL;
  const int c = c0 + 4 * q;
  const bool cok = c < C;
  const int h0 = g.h[0], w0 = g.w[0];
  int l = 0, i = (int)(gridDim.x - 1 - blockIdx.x);        // row i of level l (the grid has sum h_l rows; the coarse rows, which
  while (l < g.total - 1 && i >= g.h[l]) i -= g.h[l++];   // gather from the most fine rows, start first)
  const int hl = g.h[l], wl = g.w[l];
  float* dst = g_mem + ((size_t)n * S + g.start[l] + (size_t)i * wl) * C + c;

  if (l >= g.used) {                                       // a level the forward did not read
    if (cok)
      for (int j = slot; j < wl; j += SLOTS) *reinterpret_cast<float4*>(dst + (size_t)j * C) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  int ylo = i, ycnt = 1;
  if (l > 0) range(rng, g.by[l], i, h0, ylo, ycnt);
  const float* my = wts + g.wy[l] + i;                     // My_l[y, i] = my[y * hl]

  // ---- A: vertical (transposed) pass of the summed gradients into u
  if (g_nchw != nullptr) {
    const int xs = threadIdx.x & 15, cs = threadIdx.x >> 4;
    for (int cc = cs; cc < SLAB; cc += NT / 16) {
      const bool ok = c0 + cc < C;
      const float* gp = g_nchw + ((size_t)(n * C + (ok ? c0 + cc : 0)) * h0) * w0;
      for (int x = xs; x < w0; x += 16) {
        float acc = 0.f;
        if (ok)
          for (int k0 = 0; k0 < ycnt; k0 += UNR) {
            float wv[UNR], v[UNR];
#pragma unroll
            for (int t = 0; t < UNR; ++t) {
              const int k = k0 + t < ycnt ? k0 + t : ycnt - 1;
              wv[t] = k0 + t < ycnt ? (l > 0 ? my[(size_t)(ylo + k) * hl] : 1.f) : 0.f;
              v[t] = gp[(size_t)(ylo + k) * w0 + x];
            }
#pragma unroll
            for (int t = 0; t < UNR; ++t) acc += wv[t] * v[t];
          }
        u[x * USTR + cc] = acc;
      }
    }
    __syncthreads();
  }
  for (int x = slot; x < w0; x += SLOTS) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g_nchw != nullptr) acc = *reinterpret_cast<const float4*>(u + x * USTR + 4 * q);
    if (g_cl != nullptr && cok)
      for (int k0 = 0; k0 < ycnt; k0 += UNR) {
        float wv[UNR];
        float4 v[UNR];
#pragma unroll
        for (int t = 0; t < UNR; ++t) {
          const int k = k0 + t < ycnt ? k0 + t : ycnt - 1;
          wv[t] = k0 + t < ycnt ? (l > 0 ? my[(size_t)(ylo + k) * hl] : 1.f) : 0.f;
          v[t] = *reinterpret_cast<const float4*>(g_cl + ((size_t)(n * h0 + ylo + k) * w0 + x) * C + c);
        }
#pragma unroll
        for (int t = 0; t < UNR; ++t) fma4(acc, wv[t], v[t]);
      }
    if (l == 0) {
      if (cok) *reinterpret_cast<float4*>(dst + (size_t)x * C) = acc;
    } else {
      *reinterpret_cast<float4*>(u + x * USTR + 4 * q) = acc;
    }
  }
  if (l == 0) return;
  __syncthreads();

  // ---- B: horizontal (transposed) pass
  if (cok)
    for (int j = slot; j < wl; j += SLOTS) {
      int lo, cnt;
      range(rng, g.bx[l], j, w0, lo, cnt);
      const float* mx = wts + g.wx[l] + j;                 // Mx_l[x, j] = mx[x * wl]
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < cnt; ++k) fma4(acc, mx[(size_t)(lo + k) * wl], *reinterpret_cast<const float4*>(u + (lo + k) * USTR + 4 * q));
      *reinterpret_cast<float4*>(dst + (size_t)j * C) = acc;
    }
}

// geom_host: 9 numbers per level: h, w, start, wy, wx, fy, fx, by, bx.  0: fine, -2000: not served, else the error code.
int make_geo(const long long* gh, int total, int used, int N, int S, int C, long long wts_len, long long rng_len, Geo& g) {
  if (gh == nullptr) return -1004;
  if (total < 1 || used < 1 || used > total) return -1005;
  if (N <= 0) return -1007;
  if (S <= 0) return -1008;
  if (C <= 0) return -1009;
  if (total > MAXL || C % 4 != 0 || N > 65535 || (C + SLAB - 1) / SLAB > 65535) return -2000;
  if ((long long)N * S * C >= (1LL << 40)) return -2000;
  g.total = total;
  g.used = used;
  long long rows = 0, tokens = 0;
  for (int l = 0; l < MAXL; ++l) {
    g.h[l] = g.w[l] = 1;
    g.start[l] = g.wy[l] = g.wx[l] = g.fy[l] = g.fx[l] = g.by[l] = g.bx[l] = 0;
  }
  for (int l = 0; l < total; ++l) {
    const long long* p = gh + 9 * l;
    const long long h = p[0], w = p[1], st = p[2];
    if (h <= 0 || w <= 0 || h > 65535 || w > 65535 || st != tokens || st + h * w > S) return -1004;     // the levels tile the tokens
    tokens += h * w;
    g.h[l] = (int)h; g.w[l] = (int)w; g.start[l] = (int)st;
    rows += h;
    if (l == 0 || l >= used) continue;
    const long long h0 = gh[0], w0 = gh[1];
    if (h > h0 || w > w0) return -2000;
    // every table of the level lies inside wts / rng
    if (p[3] < 0 || p[3] + h0 * h > wts_len || p[4] < 0 || p[4] + w0 * w > wts_len) return -1004;
    if (p[5] < 0 || p[5] + 2 * h0 > rng_len || p[6] < 0 || p[6] + 2 * w0 > rng_len) return -1004;
    if (p[7] < 0 || p[7] + 2 * h > rng_len || p[8] < 0 || p[8] + 2 * w > rng_len) return -1004;
    if (wts_len >= (1LL << 31) || rng_len >= (1LL << 31)) return -1004;
    g.wy[l] = (int)p[3]; g.wx[l] = (int)p[4]; g.fy[l] = (int)p[5]; g.fx[l] = (int)p[6]; g.by[l] = (int)p[7]; g.bx[l] = (int)p[8];
  }
  if (tokens != S) return -1004;
  if (rows > 0x7fffffffLL || (long long)N * C * g.h[0] * g.w[0] >= (1LL << 40)) return -2000;
  return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ocpg_memfuse_fwd_f32(const float* memory, const float* wts, const int* rng, const long long* geom_host, long long wts_len,
                                    long long rng_len, int n_lvl_total, int n_lvl, int N, int S, int C, float* out_nchw, float* out_cl,
                                    void* stream) {
  if (memory == nullptr || !aligned16(memory)) return -1001;
  if (n_lvl > 1 && (wts == nullptr || rng == nullptr)) return -1002;
  Geo g;
  const int rc = make_geo(geom_host, n_lvl_total, n_lvl, N, S, C, wts_len, rng_len, g);
  if (rc != 0) return rc;
  if (out_nchw == nullptr && out_cl == nullptr) return -1012;
  if (out_cl != nullptr && !aligned16(out_cl)) return -1013;
  const int w0 = g.w[0];
  int tstr = w0;
  while (tstr % 16 != 1) ++tstr;
  long long floats = out_nchw != nullptr ? (long long)SLAB * tstr : 0;
  for (int l = 1; l < n_lvl; ++l) floats += (long long)g.w[l] * SLAB;
  if (floats * 4 > MAX_LDS) return -2000;
  dim3 grid(g.h[0], (C + SLAB - 1) / SLAB, N);
  hipLaunchKernelGGL(k_memfuse_fwd, grid, dim3(NT), (size_t)floats * 4, (hipStream_t)stream, memory, wts, rng, g, S, C, tstr, out_nchw,
                     out_cl);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int ocpg_memfuse_bwd_f32(const float* g_nchw, const float* g_cl, const float* wts, const int* rng, const long long* geom_host,
                                    long long wts_len, long long rng_len, int n_lvl_total, int n_lvl, int N, int S, int C, float* g_memory,
                                    void* stream) {
  if (g_nchw == nullptr && g_cl == nullptr) return -1001;
  if (g_cl != nullptr && !aligned16(g_cl)) return -1001;
  if (n_lvl > 1 && (wts == nullptr || rng == nullptr)) return -1002;
  Geo g;
  const int rc = make_geo(geom_host, n_lvl_total, n_lvl, N, S, C, wts_len, rng_len, g);
  if (rc != 0) return rc;
  if (g_memory == nullptr || !aligned16(g_memory)) return -1012;
  const long long bytes = (long long)g.w[0] * USTR * 4;
  if (bytes > MAX_LDS) return -2000;
  long long rows = 0;
  for (int l = 0; l < n_lvl_total; ++l) rows += g.h[l];
  dim3 grid((unsigned)rows, (C + SLAB - 1) / SLAB, N);
  hipLaunchKernelGGL(k_memfuse_bwd, grid, dim3(NT), (size_t)bytes, (hipStream_t)stream, g_nchw, g_cl, wts, rng, g, S, C, g_memory);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

namespace {

// ------------------------------------------------------------------------------------------------------------------------------------
// Level-set feature stack: ls_features [N, 12, Ho, Wo] = (bilinear frames 0-2, bilinear lsf 3-10, sim 11) in one launch, and its backward.
//
// The torch lines it stands for (models/ocpg.py): bilinear_resize(lsf, x4, align_corners=True), ls_feat * txt summed over the 8 channels
// divided by (normalize(ls_feat) . normalize(txt) + 1e-5) (F.normalize clamps the norm at 1e-12), bilinear_resize of the input frames,
// cat.  The two-tap tables come from resample.bilinear_matrix (per output index the first source index and the two matrix entries; the
// second tap is the next index, clamped, with weight 0 where the matrix has one entry), so the taps are the matmuls' operands.
// lsf is channels-last [N, h, w, 8] in fp32, bf16 or fp16 (dt 0 / 1 / 2) and is widened on load; everything else is fp32.
//
// Forward: a thread owns one output pixel, lanes along x: 4 x 8-channel loads of lsf, 4 x 3 of the frames, 12 coalesced stores.
// Backward, one launch, two kinds of workgroups:
//   gather   a thread owns (frame, channel c, low-res pixel): it collects wy * wx * (g[3 + c] + g[11] * dsim/df_c) from the bounded
//            window of fine pixels whose tap lands on it (by / bx ranges; the weight of a fine index for this source index is read back
//            from the two-tap tables, so it is the matrix entry).  dsim/df needs the interpolated vector f of the fine pixel: it is
//            recomputed, and only where g[11] is not zero.  No atomics.
//   txt      the workgroups after the gather ones walk the fine pixels of one clip, accumulate g[11] * dsim/dtxt where g[11] is not
//            zero and leave one 8-vector per workgroup in part [B, parts, 8]; the caller sums the parts.  A zero g[11] gives exact zeros.
constexpr int LC = 8;              // channels of lsf

struct LsTab {                     // device tables
  const int* ly_i; const float* ly_w;     // [Ho], [Ho, 2]: lsf rows
  const int* lx_i; const float* lx_w;     // [Wo], [Wo, 2]
  const int* fy_i; const float* fy_w;     // frames rows
  const int* fx_i; const float* fx_w;
  const int* by; const int* bx;           // [h, 2], [w, 2]: fine rows / columns that touch a source row / column
};

__device__ __forceinline__ void load8(const void* __restrict__ base, int dt, size_t pix, float* f) {
  if (dt == 0) {
    const float4* p = reinterpret_cast<const float4*>(base) + pix * 2;
    const float4 a = p[0], b = p[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    const uint4 r = reinterpret_cast<const uint4*>(base)[pix];
    const unsigned v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (dt == 1) {
        f[2 * k] = __uint_as_float(v[k] << 16);
        f[2 * k + 1] = __uint_as_float(v[k] & 0xffff0000u);
      } else {
        f[2 * k] = __half2float(__ushort_as_half((unsigned short)(v[k] & 0xffffu)));
        f[2 * k + 1] = __half2float(__ushort_as_half((unsigned short)(v[k] >> 16)));
      }
    }
  }
}

// f[8] = the bilinear value of lsf at fine pixel (Y, X) of frame n: horizontal taps first, then vertical (the order of the matmuls)
__device__ __forceinline__ void interp8(const void* __restrict__ lsf, int dt, const LsTab& t, int n, int h, int w, int Y, int X, float* f) {
  const int y0 = clampi(t.ly_i[Y], 0, h - 1), y1 = y0 + 1 < h ? y0 + 1 : h - 1;
  const int x0 = clampi(t.lx_i[X], 0, w - 1), x1 = x0 + 1 < w ? x0 + 1 : w - 1;
  const float wy0 = t.ly_w[2 * Y], wy1 = t.ly_w[2 * Y + 1], wx0 = t.lx_w[2 * X], wx1 = t.lx_w[2 * X + 1];
  float a[LC], b[LC], c[LC], d[LC];
  const size_t base = (size_t)n * h * w;
  load8(lsf, dt, base + (size_t)y0 * w + x0, a);
  load8(lsf, dt, base + (size_t)y0 * w + x1, b);
  load8(lsf, dt, base + (size_t)y1 * w + x0, c);
  load8(lsf, dt, base + (size_t)y1 * w + x1, d);
#pragma unroll
  for (int k = 0; k < LC; ++k) f[k] = wy0 * (wx0 * a[k] + wx1 * b[k]) + wy1 * (wx0 * c[k] + wx1 * d[k]);
}

struct Sim {                       // what sim and its derivatives need at one pixel
  float dot, nf, nt, cosv, den;    // f . t, max(|f|, 1e-12), max(|t|, 1e-12), f^ . t^, cos + 1e-5
  bool ff, tf;                     // |f|, |t| above the clamp
};

__device__ __forceinline__ Sim sim_of(const float* f, const float* t) {
  Sim s;
  float dot = 0.f, ff = 0.f, tt = 0.f;
#pragma unroll
  for (int k = 0; k < LC; ++k) { dot += f[k] * t[k]; ff += f[k] * f[k]; tt += t[k] * t[k]; }
  const float nf = sqrtf(ff), nt = sqrtf(tt);
  s.ff = nf > 1e-12f; s.tf = nt > 1e-12f;
  s.nf = s.ff ? nf : 1e-12f; s.nt = s.tf ? nt : 1e-12f;
  float cosv = 0.f;
#pragma unroll
  for (int k = 0; k < LC; ++k) cosv += (f[k] / s.nf) * (t[k] / s.nt);
  s.dot = dot; s.cosv = cosv; s.den = cosv + 1e-5f;
  return s;
}

// d sim / d a_c for a = f (other = t) or a = t (other = f): other_c / den - dot / den^2 * d cos / d a_c,
// d cos / d a_c = (other^_c - cos * a^_c) / |a| above the clamp, other^_c / 1e-12 below it
__device__ __forceinline__ float dsim(const Sim& s, float a_c, float o_c, float na, float no, bool afree) {
  const float dcos = afree ? ((o_c / no) - s.cosv * (a_c / na)) / na : (o_c / no) / na;
  return o_c / s.den - s.dot / (s.den * s.den) * dcos;
}

__global__ __launch_bounds__(NT) void k_lsfeat_fwd(const void* __restrict__ lsf, int dt, const float* __restrict__ txt,
                                                   const float* __restrict__ frames, LsTab t, int T, int h, int w, int H, int W, int Ho, int Wo,
                                                   float* __restrict__ out) {
  const int p = blockIdx.x * NT + threadIdx.x, n = blockIdx.y;
  if (p >= Ho * Wo) return;
  const int Y = p / Wo, X = p - Y * Wo;
  float* o = out + (size_t)n * 12 * Ho * Wo + p;
  const size_t plane = (size_t)Ho * Wo;
  {
    const int y0 = clampi(t.fy_i[Y], 0, H - 1), y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const int x0 = clampi(t.fx_i[X], 0, W - 1), x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const float wy0 = t.fy_w[2 * Y], wy1 = t.fy_w[2 * Y + 1], wx0 = t.fx_w[2 * X], wx1 = t.fx_w[2 * X + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* fp = frames + ((size_t)n * 3 + c) * H * W;
      o[c * plane] = wy0 * (wx0 * fp[(size_t)y0 * W + x0] + wx1 * fp[(size_t)y0 * W + x1]) +
                     wy1 * (wx0 * fp[(size_t)y1 * W + x0] + wx1 * fp[(size_t)y1 * W + x1]);
    }
  }
  float f[LC], tv[LC];
  interp8(lsf, dt, t, n, h, w, Y, X, f);
#pragma unroll
  for (int k = 0; k < LC; ++k) { tv[k] = txt[(n / T) * LC + k]; o[(3 + k) * plane] = f[k]; }
  const Sim s = sim_of(f, tv);
  o[11 * plane] = s.dot / s.den;
}

__global__ __launch_bounds__(NT) void k_lsfeat_bwd(const float* __restrict__ g, const void* __restrict__ lsf, int dt, const float* __restrict__ txt,
                                                   LsTab t, int N, int T, int h, int w, int Ho, int Wo, int gather_blocks, int parts,
                                                   float* __restrict__ g_lsf, float* __restrict__ part) {
  const size_t plane = (size_t)Ho * Wo;
  if ((int)blockIdx.x < gather_blocks) {
    const long long id = (long long)blockIdx.x * NT + threadIdx.x;       // (n, c, y, x), x fastest
    if (id >= (long long)N * LC * h * w) return;
    const int x = (int)(id % w), y = (int)((id / w) % h), c = (int)((id / ((long long)w * h)) % LC), n = (int)(id / ((long long)w * h * LC));
    int r0, rc, c0, cc;
    range(t.by, 0, y, Ho, r0, rc);
    range(t.bx, 0, x, Wo, c0, cc);
    const float* gp = g + (size_t)n * 12 * plane;
    float tv[LC];
#pragma unroll
    for (int k = 0; k < LC; ++k) tv[k] = txt[(n / T) * LC + k];
    float acc = 0.f;
    for (int Y = r0; Y < r0 + rc; ++Y) {
      const int i0 = clampi(t.ly_i[Y], 0, h - 1), i1 = i0 + 1 < h ? i0 + 1 : h - 1;
      const float wy = (i0 == y ? t.ly_w[2 * Y] : 0.f) + (i1 == y ? t.ly_w[2 * Y + 1] : 0.f);
      float row = 0.f;
      for (int X = c0; X < c0 + cc; ++X) {
        const int j0 = clampi(t.lx_i[X], 0, w - 1), j1 = j0 + 1 < w ? j0 + 1 : w - 1;
        const float wx = (j0 == x ? t.lx_w[2 * X] : 0.f) + (j1 == x ? t.lx_w[2 * X + 1] : 0.f);
        float gv = gp[(3 + c) * plane + (size_t)Y * Wo + X];
        const float g11 = gp[11 * plane + (size_t)Y * Wo + X];
        if (g11 != 0.f) {
          float f[LC];
          interp8(lsf, dt, t, n, h, w, Y, X, f);
          const Sim s = sim_of(f, tv);
          float fc = f[0], tc = tv[0];
#pragma unroll
          for (int k = 1; k < LC; ++k) if (k == c) { fc = f[k]; tc = tv[k]; }
          gv += g11 * dsim(s, fc, tc, s.nf, s.nt, s.ff);
        }
        row += wx * gv;
      }
      acc += wy * row;
    }
    g_lsf[((size_t)n * h * w + (size_t)y * w + x) * LC + c] = acc;
    return;
  }
  // ---- txt: workgroup `pi` of clip b
  __shared__ float red[NT];
  const int bi = ((int)blockIdx.x - gather_blocks) / parts, pi = ((int)blockIdx.x - gather_blocks) % parts;
  float tv[LC], acc[LC];
#pragma unroll
  for (int k = 0; k < LC; ++k) { tv[k] = txt[bi * LC + k]; acc[k] = 0.f; }
  const long long total = (long long)T * (long long)plane;
  for (long long p = (long long)pi * NT + threadIdx.x; p < total; p += (long long)parts * NT) {
    const int n = bi * T + (int)(p / (long long)plane);
    const int q = (int)(p % (long long)plane), Y = q / Wo, X = q - Y * Wo;
    const float g11 = g[((size_t)n * 12 + 11) * plane + q];
    if (g11 != 0.f) {
      float f[LC];
      interp8(lsf, dt, t, n, h, w, Y, X, f);
      const Sim s = sim_of(f, tv);
#pragma unroll
      for (int k = 0; k < LC; ++k) acc[k] += g11 * dsim(s, tv[k], f[k], s.nt, s.nf, s.tf);
    }
  }
#pragma unroll
  for (int k = 0; k < LC; ++k) {
    red[threadIdx.x] = acc[k];
    __syncthreads();
    for (int st = NT / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[((size_t)bi * parts + pi) * LC + k] = red[0];
    __syncthreads();
  }
}

int ls_check(const void* lsf, int dt, const float* txt, const void* tab_i, const void* tab_w, const long long* off, int B, int T, int h, int w,
             int H, int W, int Ho, int Wo) {
  if (lsf == nullptr || !aligned16(lsf)) return -1001;
  if (dt < 0 || dt > 2) return -1002;
  if (txt == nullptr) return -1003;
  if (tab_i == nullptr || tab_w == nullptr || off == nullptr) return -1004;
  if (B <= 0 || T <= 0) return -1005;
  if (h <= 0 || w <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return -1006;
  if ((long long)B * T > 65535 || (long long)Ho * Wo >= (1LL << 31) || (long long)B * T * 12 * Ho * Wo >= (1LL << 40) ||
      (long long)B * T * LC * h * w >= (1LL << 31) * (long long)NT)
    return -2000;
  return 0;
}

// off (host): int offsets of ly_i, lx_i, fy_i, fx_i, by, bx in tab_i, then float offsets of ly_w, lx_w, fy_w, fx_w in tab_w, then the
// lengths of tab_i and tab_w: 12 numbers
int ls_tab(const int* tab_i, const float* tab_w, const long long* off, int h, int w, int Ho, int Wo, LsTab& t) {
  const long long ni = off[10], nw = off[11];
  const long long need_i[6] = {Ho, Wo, Ho, Wo, 2LL * h, 2LL * w}, need_w[4] = {2LL * Ho, 2LL * Wo, 2LL * Ho, 2LL * Wo};
  for (int k = 0; k < 6; ++k) if (off[k] < 0 || off[k] + need_i[k] > ni) return -1004;
  for (int k = 0; k < 4; ++k) if (off[6 + k] < 0 || off[6 + k] + need_w[k] > nw) return -1004;
  t.ly_i = tab_i + off[0]; t.lx_i = tab_i + off[1]; t.fy_i = tab_i + off[2]; t.fx_i = tab_i + off[3];
  t.by = tab_i + off[4]; t.bx = tab_i + off[5];
  t.ly_w = tab_w + off[6]; t.lx_w = tab_w + off[7]; t.fy_w = tab_w + off[8]; t.fx_w = tab_w + off[9];
  return 0;
}

}  // namespace

extern "C" int ocpg_lsfeat_fwd_f32(const void* lsf, int lsf_dtype, const float* txt, const float* frames, const int* tab_i, const float* tab_w,
                                   const long long* off_host, int B, int T, int h, int w, int H, int W, int Ho, int Wo, float* out,
                                   void* stream) {
  int rc = ls_check(lsf, lsf_dtype, txt, tab_i, tab_w, off_host, B, T, h, w, H, W, Ho, Wo);
  if (rc != 0) return rc;
  if (frames == nullptr) return -1007;
  if (out == nullptr) return -1012;
  LsTab t;
  rc = ls_tab(tab_i, tab_w, off_host, h, w, Ho, Wo, t);
  if (rc != 0) return rc;
  dim3 grid((unsigned)(((long long)Ho * Wo + NT - 1) / NT), (unsigned)(B * T));
  hipLaunchKernelGGL(k_lsfeat_fwd, grid, dim3(NT), 0, (hipStream_t)stream, lsf, lsf_dtype, txt, frames, t, T, h, w, H, W, Ho, Wo, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int ocpg_lsfeat_bwd_parts(int T, int Ho, int Wo) {
  const long long per = ((long long)T * Ho * Wo + 4095) / 4096;
  return (int)(per < 1 ? 1 : (per > 128 ? 128 : per));
}

extern "C" int ocpg_lsfeat_bwd_f32(const float* g, const void* lsf, int lsf_dtype, const float* txt, const int* tab_i, const float* tab_w,
                                   const long long* off_host, int B, int T, int h, int w, int Ho, int Wo, float* g_lsf, float* g_txt_part,
                                   void* stream) {
  int rc = ls_check(lsf, lsf_dtype, txt, tab_i, tab_w, off_host, B, T, h, w, 1, 1, Ho, Wo);
  if (rc != 0) return rc;
  if (g == nullptr) return -1007;
  if (g_lsf == nullptr || g_txt_part == nullptr) return -1012;
  LsTab t;
  rc = ls_tab(tab_i, tab_w, off_host, h, w, Ho, Wo, t);
  if (rc != 0) return rc;
  const int parts = ocpg_lsfeat_bwd_parts(T, Ho, Wo);
  const long long gather = ((long long)B * T * LC * h * w + NT - 1) / NT;
  hipLaunchKernelGGL(k_lsfeat_bwd, dim3((unsigned)(gather + (long long)B * parts)), dim3(NT), 0, (hipStream_t)stream, g, lsf, lsf_dtype, txt, t,
                     B * T, T, h, w, Ho, Wo, (int)gather, parts, g_lsf, g_txt_part);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
