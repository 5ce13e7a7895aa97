// Weak-annotation similarity head (reference pre_process/sim_model.py:35-134; semantics in include/ocpg_hip.h).
//
// Per object o on frame f with candidates c (feature cells) and the frame's pixels p:
//   a_c[p] = k^_c . k^_p,  s_c[p] = (a_c[p] - min_p a_c) / max_p a_c,  score_c = soft IoU of s_c's row / column maxima with the box,
//   heat[o] = s of the best candidate.
// The product [n, C] x [C, h*w] is the work; everything else is O(n * h*w).  Four launches:
//   1. sim_inv_norm  a wave per pixel: 1 / |feat[f, p]|, channels read as float4.
//   2. sim_rows      the product as a register-tiled fp32 GEMM: a 256-thread workgroup owns 64 candidates of one object x 64 pixels,
//                    walks C in steps of 16 through LDS (both operands K-contiguous in memory, stored transposed so a thread reads
//                    its 4 candidates / 4 pixels as one float4), 4x4 accumulators per thread.  The epilogue scales by the two inverse
//                    norms and writes rows[c][p] (workspace).  A key vector is read once per 64 candidates.
//   3. sim_reduce    a workgroup per candidate: its row in LDS (h*w <= 8192), min / max, then the box score from column maxima (a
//                    thread per column) and row maxima (a wave per row).  Rounding is monotone, so max_y s = (max_y a - min) / max
//                    exactly: the maxima are taken on a and rescaled once.
//   4. sim_select    a workgroup per object: the best score (lowest index among equals), choice, and the rescaled plane.
// Sums run in a fixed order (per-thread partials, shuffle tree, 4 waves in order); no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int TM = 64;           // candidates per tile
constexpr int TN = 64;           // pixels per tile
constexpr int KC = 16;           // channels per LDS step
constexpr int LDP = TM + 4;      // padded LDS row: the transposed stores of a wave spread over the banks, float4 reads stay aligned
constexpr int MAXC = 256;        // candidates per object
constexpr int MAXP = 8192;       // h*w: one row in LDS

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// candidates [c0, c0 + n) of object o, read from device memory and forced into [0, total], n <= MAXC
__device__ __forceinline__ void object_range(const int* __restrict__ cand_off, int o, int total, int& c0, int& n) {
  c0 = clampi(cand_off[o], 0, total);
  const int c1 = clampi(cand_off[o + 1], c0, total);
  n = c1 - c0 < MAXC ? c1 - c0 : MAXC;
}

__global__ __launch_bounds__(NT) void sim_inv_norm(const float* __restrict__ feat, long long npix, int C, float* __restrict__ invn) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (p >= npix) return;                                               // uniform over the wave
  const float4* v = reinterpret_cast<const float4*>(feat + p * C);
  float s = 0.f;
  for (int k = lane; k < C / 4; k += 64) {
    const float4 t = v[k];
    s = fmaf(t.x, t.x, s);
    s = fmaf(t.y, t.y, s);
    s = fmaf(t.z, t.z, s);
    s = fmaf(t.w, t.w, s);
  }
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) invn[p] = 1.0f / sqrtf(s);
}

__global__ __launch_bounds__(NT) void sim_rows(const float* __restrict__ feat, const float* __restrict__ invn, int F, int h, int w, int C,
                                               int total, const int* __restrict__ obj_frame, const int* __restrict__ cand_off,
                                               const int* __restrict__ cand_xy, float* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) float As[KC][LDP];
  __shared__ __attribute__((aligned(16))) float Bs[KC][LDP];
  const int P = h * w;
  const int o = blockIdx.z;
  int c0, n;
  object_range(cand_off, o, total, c0, n);
  const int m0 = blockIdx.y * TM;
  if (m0 >= n) return;                                                 // uniform over the workgroup
  const int p0 = blockIdx.x * TN;
  const int f = clampi(obj_frame[o], 0, F - 1);
  const float* base = feat + (long long)f * P * C;
  const float* nbase = invn + (long long)f * P;

  const int tid = threadIdx.x;
  const int lr = tid >> 2, lk = (tid & 3) * 4;                         // the row and the 4 channels this thread stages
  const float* arow = nullptr;
  if (m0 + lr < n) {
    const int* xy = cand_xy + 2ll * (c0 + m0 + lr);
    arow = base + (long long)(clampi(xy[1], 0, h - 1) * w + clampi(xy[0], 0, w - 1)) * C;
  }
  const float* brow = p0 + lr < P ? base + (long long)(p0 + lr) * C : nullptr;

  const int ty = tid >> 4, tx = tid & 15;                              // 4 candidates x 4 pixels per thread
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  for (int k0 = 0; k0 < C; k0 += KC) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (k0 + lk < C) {                                                 // C % 4 == 0: a float4 is inside or outside as a whole
      if (arow) a = *reinterpret_cast<const float4*>(arow + k0 + lk);
      if (brow) b = *reinterpret_cast<const float4*>(brow + k0 + lk);
    }
    __syncthreads();                                                   // the previous step's reads are done
    As[lk + 0][lr] = a.x;
    As[lk + 1][lr] = a.y;
    As[lk + 2][lr] = a.z;
    As[lk + 3][lr] = a.w;
    Bs[lk + 0][lr] = b.x;
    Bs[lk + 1][lr] = b.y;
    Bs[lk + 2][lr] = b.z;
    Bs[lk + 3][lr] = b.w;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const float4 av = *reinterpret_cast<const float4*>(&As[k][ty * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&Bs[k][tx * 4]);
      const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], br[j], acc[i][j]);
    }
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty * 4 + i;
    if (m >= n) continue;
    const int* xy = cand_xy + 2ll * (c0 + m);
    const float nq = nbase[clampi(xy[1], 0, h - 1) * w + clampi(xy[0], 0, w - 1)];
    float* out = rows + (long long)(c0 + m) * P;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + tx * 4 + j;
      if (p < P) out[p] = acc[i][j] * nq * nbase[p];
    }
  }
}

// sum / min / max over the workgroup in a fixed order; every thread gets the result.  red: NT / 64 floats of LDS
template <int OP>
__device__ __forceinline__ float block_reduce(float v, float* red) {
  for (int o = 32; o; o >>= 1) {
    const float u = __shfl_xor(v, o);
    v = OP == 0 ? v + u : (OP == 1 ? fminf(v, u) : fmaxf(v, u));
  }
  __syncthreads();                                                     // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < NT / 64; ++i) r = OP == 0 ? r + red[i] : (OP == 1 ? fminf(r, red[i]) : fmaxf(r, red[i]));
  return r;
}

// grid (max candidates of an object, n_obj).  mnmx [total, 2], score_out [total]
__global__ __launch_bounds__(NT) void sim_reduce(const float* __restrict__ rows, int h, int w, int total, const int* __restrict__ cand_off,
                                                 const int* __restrict__ box, float* __restrict__ mnmx, float* __restrict__ score_ws,
                                                 float* __restrict__ score) {
  __shared__ float row[MAXP];
  __shared__ float red[NT / 64];
  const int o = blockIdx.y;
  int c0, n;
  object_range(cand_off, o, total, c0, n);
  if ((int)blockIdx.x >= n) return;                                    // uniform over the workgroup
  const int c = c0 + blockIdx.x;
  const int P = h * w, tid = threadIdx.x;
  const float* src = rows + (long long)c * P;
  float lo = INFINITY, hi = -INFINITY;
  for (int p = tid; p < P; p += NT) {
    const float v = src[p];
    row[p] = v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  const float mn = block_reduce<1>(lo, red);                           // its barriers also publish row[]
  const float mx = block_reduce<2>(hi, red);
  float sc = 0.f;
  if (box) {
    const int x0 = box[4 * o], y0 = box[4 * o + 1], x1 = box[4 * o + 2], y1 = box[4 * o + 3];
    float nx = 0.f, dx = 0.f, ny = 0.f, dy = 0.f;
    for (int x = tid; x < w; x += NT) {                                // column maxima: a thread per column
      float m = row[x];
      for (int y = 1; y < h; ++y) m = fmaxf(m, row[y * w + x]);
      const float s = (m - mn) / mx, b = (x >= x0 && x < x1) ? 1.f : 0.f;
      nx += s * b;
      dx += s + b - s * b;
    }
    const int lane = tid & 63;
    for (int y = tid >> 6; y < h; y += NT / 64) {                      // row maxima: a wave per row
      float m = -INFINITY;
      for (int x = lane; x < w; x += 64) m = fmaxf(m, row[y * w + x]);
      for (int s = 32; s; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
      if (lane == 0) {
        const float s = (m - mn) / mx, b = (y >= y0 && y < y1) ? 1.f : 0.f;
        ny += s * b;
        dy += s + b - s * b;
      }
    }
    nx = block_reduce<0>(nx, red);
    dx = block_reduce<0>(dx, red);
    ny = block_reduce<0>(ny, red);
    dy = block_reduce<0>(dy, red);
    sc = 0.5f * (nx / (dx + 1e-5f) + ny / (dy + 1e-5f));
  }
  if (tid == 0) {
    mnmx[2ll * c] = mn;
    mnmx[2ll * c + 1] = mx;
    score_ws[c] = sc;
    if (score) score[c] = sc;
  }
}

// grid n_obj
__global__ __launch_bounds__(NT) void sim_select(const float* __restrict__ rows, int P, int total, const int* __restrict__ cand_off,
                                                 const float* __restrict__ mnmx, const float* __restrict__ score_ws,
                                                 float* __restrict__ heat, int* __restrict__ choice) {
  __shared__ float sv[NT];
  __shared__ int si[NT];
  const int o = blockIdx.x, tid = threadIdx.x;
  int c0, n;
  object_range(cand_off, o, total, c0, n);
  float* out = heat + (long long)o * P;
  if (n == 0) {                                                        // uniform over the workgroup
    for (int p = tid; p < P; p += NT) out[p] = 0.f;
    if (tid == 0) choice[o] = -1;
    return;
  }
  sv[tid] = tid < n ? score_ws[c0 + tid] : -INFINITY;                  // NT == MAXC: a thread per candidate
  si[tid] = tid < n ? tid : MAXC;
  __syncthreads();
  for (int s = NT / 2; s; s >>= 1) {
    if (tid < s) {
      const float a = sv[tid], b = sv[tid + s];
      const int ia = si[tid], ib = si[tid + s];
      if (b > a || (b == a && ib < ia)) {
        sv[tid] = b;
        si[tid] = ib;
      }
    }
    __syncthreads();
  }
  const int best = si[0] < n ? si[0] : 0;
  const float mn = mnmx[2ll * (c0 + best)], mx = mnmx[2ll * (c0 + best) + 1];
  const float* src = rows + (long long)(c0 + best) * P;
  for (int p = tid; p < P; p += NT) out[p] = (src[p] - mn) / mx;
  if (tid == 0) choice[o] = best;
}

static_assert(NT == MAXC, "sim_select gives every candidate of an object a thread");

// workspace layout in floats: inverse norms [F*P] | rows [total*P] | min/max [2*total] | scores [total], each part a multiple of 4
inline long long pad4(long long v) { return (v + 3) & ~3ll; }

}  // namespace

extern "C" long long ocpg_sim_heat_workspace(int F, int h, int w, int total) {
  if (F <= 0 || h <= 0 || w <= 0 || total < 0) return 0;
  const long long P = (long long)h * w;
  return 4 * (pad4(F * P) + pad4(total * P) + pad4(2ll * total) + pad4(total));
}

extern "C" int ocpg_sim_heat_f32(const float* feat, int F, int h, int w, int C, int n_obj, const int* obj_frame, const int* cand_off_host,
                                 const int* cand_off, const int* cand_xy, const int* box, float* heat, int* choice, float* score,
                                 void* workspace, void* stream) {
  if (!feat || ((uintptr_t)feat & 15)) return -1001;
  if (F <= 0) return -1002;
  if (h <= 0) return -1003;
  if (w <= 0 || (long long)h * w > MAXP || (long long)F * h * w >= (1ll << 31)) return -1004;
  if (C <= 0 || C % 4 != 0) return -1005;
  if (n_obj <= 0 || n_obj > 65535) return -1006;
  if (!obj_frame) return -1007;
  if (!cand_off_host || cand_off_host[0] != 0) return -1008;
  int max_n = 0;
  for (int o = 0; o < n_obj; ++o) {
    const int n = cand_off_host[o + 1] - cand_off_host[o];
    if (n < 0 || n > MAXC) return -1008;
    if (n > max_n) max_n = n;
  }
  const int total = cand_off_host[n_obj];
  if (!cand_off) return -1009;
  if (!cand_xy && total > 0) return -1010;
  if (!heat) return -1012;
  if (!choice) return -1013;
  if (!workspace || ((uintptr_t)workspace & 15)) return -1015;

  const int P = h * w;
  const long long npix = (long long)F * P;
  float* invn = (float*)workspace;
  float* rows = invn + pad4(npix);
  float* mnmx = rows + pad4((long long)total * P);
  float* score_ws = mnmx + pad4(2ll * total);
  hipStream_t st = (hipStream_t)stream;
  if (max_n > 0) {
    sim_inv_norm<<<(unsigned)((npix + NT / 64 - 1) / (NT / 64)), NT, 0, st>>>(feat, npix, C, invn);
    sim_rows<<<dim3((unsigned)((P + TN - 1) / TN), (unsigned)((max_n + TM - 1) / TM), (unsigned)n_obj), NT, 0, st>>>(
        feat, invn, F, h, w, C, total, obj_frame, cand_off, cand_xy, rows);
    sim_reduce<<<dim3((unsigned)max_n, (unsigned)n_obj), NT, 0, st>>>(rows, h, w, total, cand_off, box, mnmx, score_ws, score);
  }
  sim_select<<<(unsigned)n_obj, NT, 0, st>>>(rows, P, total, cand_off, mnmx, score_ws, heat, choice);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
