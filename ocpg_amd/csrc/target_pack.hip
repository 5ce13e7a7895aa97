// Everything the matcher and the criterion derive from the batch's targets alone, in two launches (semantics in include/ocpg_hip.h,
// DESIGN.md 4.8t; the torch composition it replaces: models/ops/functions/target_pack_func.py).
//
//   1. tp_pack       grid (segments, clips of the chunk).  The clip's pointers and extents arrive by value in the kernel arguments
//                    (no pointer table in device memory, nothing to copy: the call can be captured into a graph).  A clip's blocks are
//                    split into five segments: the stride-s maps (gt, region, weak * region, folded heat), the stride-sl maps (region,
//                    weak * region, folded heat), the matcher's stride-sm gt, the nearest-resized region, and one block for the
//                    [B, T] rows (boxes, valid, labels).  A thread owns 4 consecutive output pixels of a row and stores 16 bytes per
//                    map; padding (rows / columns past the clip's own extent) is written as zero, so no output is pre-zeroed.  The
//                    box is rasterised from its bounds (a few integer compares per pixel), never read back from another output.
//                    Each block of the two heat segments leaves the min / max of its folded heat in the workspace.
//   2. tp_normalise  every block folds all partials of its map (a few hundred) and normalises the folded heat in place:
//                    (a - lo) / (hi - lo + 1e-5), 1 where the region is 0.
// With more than 16 clips the host issues tp_pack once per chunk of 16 and tp_normalise once over all of them.
// min / max are order-independent: no atomics, the same bits on every call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int MAXB = 16;         // clips per launch
constexpr int NORM_BLOCKS = 1024;  // tp_normalise: blocks per map at most

struct Clips {
  const float* masks[MAXB];
  const float* heat[MAXB];
  const float* weak[MAXB];
  const float* boxes[MAXB];
  const long long* valid[MAXB];
  const long long* labels[MAXB];
  const long long* size[MAXB];
  int H[MAXB], W[MAXB];
};

struct Outs {
  float *gt_s, *gt_m, *region_s, *region_l, *region_ls, *weak_s, *weak_l, *w_s, *w_l, *tboxes, *valid_f;
  long long *valid_i, *labels;
};

struct Geo {
  int T, PH, PW, s, sl, sm, lh, lw;
  int nb_s, nb_l, nb_m, nb_r;    // blocks per clip of the four map segments
  int clip0;                     // first clip of this chunk
};

struct Box {
  int x0, x1, y0, y1;            // empty (all zero) when the truncated box has no area
};

// Python's start:stop on an axis of length size (models/segmentation.py:_py_slice_bounds)
__device__ __forceinline__ int slice_bound(int v, int size) { return v < 0 ? max(v + size, 0) : min(v, size); }

__device__ __forceinline__ Box raster_box(const float* __restrict__ b, const long long* __restrict__ size, int PH, int PW) {
  const float cx = b[0], cy = b[1], w = b[2], h = b[3];
  const float fh = (float)size[0], fw = (float)size[1];
  const int sx0 = (int)(fmaf(w, -0.5f, cx) * fw), sy0 = (int)(fmaf(h, -0.5f, cy) * fh);
  const int sx1 = (int)(fmaf(w, 0.5f, cx) * fw), sy1 = (int)(fmaf(h, 0.5f, cy) * fh);
  Box r = {0, 0, 0, 0};
  if ((int)((unsigned)sy1 - (unsigned)sy0) > 0 && (int)((unsigned)sx1 - (unsigned)sx0) > 0) {
    r.x0 = slice_bound(sx0, PW);
    r.x1 = slice_bound(sx1, PW);
    r.y0 = slice_bound(sy0, PH);
    r.y1 = slice_bound(sy1, PH);
  }
  return r;
}

__device__ __forceinline__ float in_box(const Box& b, int y, int x) { return (y >= b.y0 && y < b.y1 && x >= b.x0 && x < b.x1) ? 1.f : 0.f; }

// |clamp(h, 0.3, 0.7) - 0.5|, NaN kept as ATen's clamp keeps it
__device__ __forceinline__ float fold_heat(float h) { return fabsf((h != h ? h : fminf(fmaxf(h, 0.3f), 0.7f)) - 0.5f); }

__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// pixels (y, x0 + j * k), j < 4, of frame t of a [T, H, W] clip; zero past the clip's extent
__device__ __forceinline__ float4 read4(const float* __restrict__ src, int t, int H, int W, int y, int x0, int k) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (y >= H) return v;
  const float* row = src + ((long long)t * H + y) * W;
  if (k == 1 && x0 + 3 < W && (((uintptr_t)(row + x0)) & 15) == 0) return *reinterpret_cast<const float4*>(row + x0);
  if (x0 < W) v.x = row[x0];
  if (x0 + k < W) v.y = row[x0 + k];
  if (x0 + 2 * k < W) v.z = row[x0 + 2 * k];
  if (x0 + 3 * k < W) v.w = row[x0 + 3 * k];
  return v;
}

__device__ __forceinline__ void store4(float* __restrict__ dst, long long off, float4 v) { *reinterpret_cast<float4*>(dst + off) = v; }

// min / max over the workgroup, every thread gets both.  red: 2 * NT / 64 floats of LDS
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* red) {
  for (int o = 32; o; o >>= 1) {
    lo = nan_min(lo, __shfl_xor(lo, o));
    hi = nan_max(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = lo;
    red[NT / 64 + (threadIdx.x >> 6)] = hi;
  }
  __syncthreads();
  lo = red[0];
  hi = red[NT / 64];
  for (int i = 1; i < NT / 64; ++i) {
    lo = nan_min(lo, red[i]);
    hi = nan_max(hi, red[NT / 64 + i]);
  }
}

// the stride-k maps of clip c (global index bc): region, weak * region and the folded heat, for k == s also gt.  part: this block's
// {min, max} slots
template <bool GT>
__device__ __forceinline__ void pack_maps(const Clips& cl, int c, long long bc, const Geo& g, int k, int blk, int nblk, float* __restrict__ gt,
                                          float* __restrict__ region, float* __restrict__ weak, float* __restrict__ wmap,
                                          float* __restrict__ pmin, float* __restrict__ pmax, float* red) {
  const int OH = g.PH / k, OW4 = g.PW / k / 4, H = cl.H[c], W = cl.W[c];
  const long long nq = (long long)g.T * OH * OW4;
  float lo = INFINITY, hi = -INFINITY;
  for (long long q = (long long)blk * NT + threadIdx.x; q < nq; q += (long long)nblk * NT) {
    const int ox = (int)(q % OW4) * 4;
    const long long r = q / OW4;
    const int oy = (int)(r % OH), t = (int)(r / OH);
    const int y = oy * k + k / 2, x = ox * k + k / 2;
    const Box b = raster_box(cl.boxes[c] + 4 * t, cl.size[c], g.PH, g.PW);
    const float4 rg = make_float4(in_box(b, y, x), in_box(b, y, x + k), in_box(b, y, x + 2 * k), in_box(b, y, x + 3 * k));
    const float4 wk = read4(cl.weak[c], t, H, W, y, x, k);
    const float4 ht = read4(cl.heat[c], t, H, W, y, x, k);
    const float4 a = make_float4(fold_heat(ht.x), fold_heat(ht.y), fold_heat(ht.z), fold_heat(ht.w));
    lo = nan_min(nan_min(nan_min(lo, a.x), nan_min(a.y, a.z)), a.w);
    hi = nan_max(nan_max(nan_max(hi, a.x), nan_max(a.y, a.z)), a.w);
    const long long off = (((bc * g.T + t) * OH + oy) * OW4) * 4 + ox;
    if (GT) store4(gt, off, read4(cl.masks[c], t, H, W, y, x, k));
    store4(region, off, rg);
    store4(weak, off, make_float4(wk.x * rg.x, wk.y * rg.y, wk.z * rg.z, wk.w * rg.w));
    store4(wmap, off, a);
  }
  block_minmax(lo, hi, red);
  if (threadIdx.x == 0) {
    *pmin = lo;
    *pmax = hi;
  }
}

// part: [min_s | max_s | min_l | max_l], np_s = B * nb_s and np_l = B * nb_l slots each (B = all clips of the call)
__global__ __launch_bounds__(NT) void tp_pack(const Clips cl, const Outs o, const Geo g, float* __restrict__ part, int np_s, int np_l) {
  __shared__ float red[2 * NT / 64];
  const int c = blockIdx.y;
  const long long bc = g.clip0 + c;
  int blk = blockIdx.x;
  if (blk < g.nb_s) {
    pack_maps<true>(cl, c, bc, g, g.s, blk, g.nb_s, o.gt_s, o.region_s, o.weak_s, o.w_s, part + bc * g.nb_s + blk,
                    part + np_s + bc * g.nb_s + blk, red);
    return;
  }
  blk -= g.nb_s;
  if (blk < g.nb_l) {
    pack_maps<false>(cl, c, bc, g, g.sl, blk, g.nb_l, nullptr, o.region_l, o.weak_l, o.w_l, part + 2ll * np_s + bc * g.nb_l + blk,
                     part + 2ll * np_s + np_l + bc * g.nb_l + blk, red);
    return;
  }
  blk -= g.nb_l;
  if (blk < g.nb_m) {                                                  // the matcher's sub-sampled ground truth
    const int k = g.sm, OH = g.PH / k, OW4 = g.PW / k / 4;
    const long long nq = (long long)g.T * OH * OW4;
    for (long long q = (long long)blk * NT + threadIdx.x; q < nq; q += (long long)g.nb_m * NT) {
      const int ox = (int)(q % OW4) * 4;
      const long long r = q / OW4;
      const int oy = (int)(r % OH), t = (int)(r / OH);
      store4(o.gt_m, (((bc * g.T + t) * OH + oy) * OW4) * 4 + ox, read4(cl.masks[c], t, cl.H[c], cl.W[c], oy * k + k / 2, ox * k + k / 2, k));
    }
    return;
  }
  blk -= g.nb_m;
  if (blk < g.nb_r) {                                                  // nearest resize of the stride-s region to (lh, lw)
    const int k = g.s, IH = g.PH / k, IW = g.PW / k, OW4 = g.lw / 4;
    const float sh = (float)IH / (float)g.lh, sw = (float)IW / (float)g.lw;
    const long long nq = (long long)g.T * g.lh * OW4;
    for (long long q = (long long)blk * NT + threadIdx.x; q < nq; q += (long long)g.nb_r * NT) {
      const int ox = (int)(q % OW4) * 4;
      const long long r = q / OW4;
      const int oy = (int)(r % g.lh), t = (int)(r / g.lh);
      const Box b = raster_box(cl.boxes[c] + 4 * t, cl.size[c], g.PH, g.PW);
      const int y = min((int)floorf(oy * sh), IH - 1) * k + k / 2;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = in_box(b, y, min((int)floorf((ox + j) * sw), IW - 1) * k + k / 2);
      store4(o.region_ls, (((bc * g.T + t) * g.lh + oy) * OW4) * 4 + ox, make_float4(v[0], v[1], v[2], v[3]));
    }
    return;
  }
  for (int t = threadIdx.x; t < g.T; t += NT) {                        // the [B, T] rows
    const long long i = bc * g.T + t;
    const long long vd = cl.valid[c][t];
    o.valid_i[i] = vd;
    o.valid_f[i] = (float)vd;
    if (o.labels) o.labels[i] = cl.labels[c][t];
    store4(o.tboxes, 4 * i, make_float4(cl.boxes[c][4 * t], cl.boxes[c][4 * t + 1], cl.boxes[c][4 * t + 2], cl.boxes[c][4 * t + 3]));
  }
}

// blocks [0, nbn_s): w_s, the rest: w_l.  n4: float4s per map
__global__ __launch_bounds__(NT) void tp_normalise(float* __restrict__ w_s, const float* __restrict__ region_s, long long n4_s, int nbn_s,
                                                   float* __restrict__ w_l, const float* __restrict__ region_l, long long n4_l,
                                                   const float* __restrict__ part, int np_s, int np_l) {
  __shared__ float red[2 * NT / 64];
  const bool low = (int)blockIdx.x >= nbn_s;
  const int blk = low ? blockIdx.x - nbn_s : blockIdx.x, nblk = low ? gridDim.x - nbn_s : nbn_s;
  const float* pmin = low ? part + 2ll * np_s : part;
  const int np = low ? np_l : np_s;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < np; i += NT) {
    lo = nan_min(lo, pmin[i]);
    hi = nan_max(hi, pmin[np + i]);
  }
  block_minmax(lo, hi, red);
  const float den = hi - lo + 1e-5f;
  float4* w = reinterpret_cast<float4*>(low ? w_l : w_s);
  const float4* rg = reinterpret_cast<const float4*>(low ? region_l : region_s);
  const long long n4 = low ? n4_l : n4_s;
  for (long long i = (long long)blk * NT + threadIdx.x; i < n4; i += (long long)nblk * NT) {
    const float4 a = w[i], r = rg[i];
    w[i] = make_float4(r.x == 0.f ? 1.f : (a.x - lo) / den, r.y == 0.f ? 1.f : (a.y - lo) / den, r.z == 0.f ? 1.f : (a.z - lo) / den,
                       r.w == 0.f ? 1.f : (a.w - lo) / den);
  }
}

inline int blocks_for(long long quads, int cap) {
  const long long b = (quads + NT - 1) / NT;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

inline int clip_cap(int B) { return 1024 / B > 32 ? 1024 / B : 32; }    // blocks per clip and segment at most

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" long long ocpg_target_pack_workspace(int B) { return B <= 0 ? 0 : 16ll * B * clip_cap(B); }

extern "C" int ocpg_target_pack_f32(int B, int T, const void* const* masks, const void* const* heat, const void* const* weak, const int* hw,
                                    const void* const* boxes, const void* const* valid, const void* const* labels, const void* const* size,
                                    int PH, int PW, int s, int sl, int sm, int lh, int lw, float* gt_s, float* gt_m, float* region_s,
                                    float* region_l, float* region_ls, float* weak_s, float* weak_l, float* w_s, float* w_l, float* tboxes,
                                    float* valid_f, long long* valid_i, long long* labels_out, void* workspace, void* stream) {
  if (B <= 0) return -1001;
  if (T <= 0) return -1002;
  if (!masks || !heat || !weak || !hw || !boxes || !valid || !size) return -1003;
  if (PH <= 0 || PW <= 0) return -1005;
  if (s <= 0 || sl <= 0 || sm <= 0) return -1006;
  if (lh <= 0 || lw <= 0) return -1007;
  for (int i = 0; i < B; ++i) {
    if (!masks[i] || !heat[i] || !weak[i] || !boxes[i] || !valid[i] || !size[i] || (labels && !labels[i])) return -1003;
    if (hw[2 * i] <= 0 || hw[2 * i] > PH || hw[2 * i + 1] <= 0 || hw[2 * i + 1] > PW) return -1004;
  }
  float* const maps[] = {gt_s, gt_m, region_s, region_l, region_ls, weak_s, weak_l, w_s, w_l, tboxes};
  for (float* p : maps)
    if (!p || misaligned(p)) return -1008;
  if (!valid_f || !valid_i || (labels && !labels_out)) return -1009;
  if (!workspace) return -1010;
  // 16-byte stores of 4 pixels of a row: every output row is a multiple of 4 wide; the sub-sampling covers the padded extent exactly
  for (int k : {s, sl, sm})
    if (PH % k != 0 || PW % (4 * k) != 0) return -2000;
  if (lw % 4 != 0) return -2000;
  if ((long long)B * T * PH * PW >= (1ll << 40) || (long long)T * PH * PW >= (1ll << 31) || (long long)T * lh * lw >= (1ll << 31)) return -2000;

  const int cap = clip_cap(B);
  Geo g;
  g.T = T, g.PH = PH, g.PW = PW, g.s = s, g.sl = sl, g.sm = sm, g.lh = lh, g.lw = lw;
  g.nb_s = blocks_for((long long)T * (PH / s) * (PW / s / 4), cap);
  g.nb_l = blocks_for((long long)T * (PH / sl) * (PW / sl / 4), cap);
  g.nb_m = blocks_for((long long)T * (PH / sm) * (PW / sm / 4), cap);
  g.nb_r = blocks_for((long long)T * lh * (lw / 4), cap);
  const int np_s = B * g.nb_s, np_l = B * g.nb_l;
  Outs o = {gt_s, gt_m, region_s, region_l, region_ls, weak_s, weak_l, w_s, w_l, tboxes, valid_f, valid_i, labels ? labels_out : nullptr};
  hipStream_t st = (hipStream_t)stream;
  for (int c0 = 0; c0 < B; c0 += MAXB) {
    const int n = B - c0 < MAXB ? B - c0 : MAXB;
    Clips cl = {};
    for (int i = 0; i < n; ++i) {
      cl.masks[i] = (const float*)masks[c0 + i];
      cl.heat[i] = (const float*)heat[c0 + i];
      cl.weak[i] = (const float*)weak[c0 + i];
      cl.boxes[i] = (const float*)boxes[c0 + i];
      cl.valid[i] = (const long long*)valid[c0 + i];
      cl.labels[i] = labels ? (const long long*)labels[c0 + i] : nullptr;
      cl.size[i] = (const long long*)size[c0 + i];
      cl.H[i] = hw[2 * (c0 + i)];
      cl.W[i] = hw[2 * (c0 + i) + 1];
    }
    g.clip0 = c0;
    tp_pack<<<dim3((unsigned)(g.nb_s + g.nb_l + g.nb_m + g.nb_r + 1), (unsigned)n), NT, 0, st>>>(cl, o, g, (float*)workspace, np_s, np_l);
  }
  const long long n4_s = (long long)B * T * (PH / s) * (PW / s / 4), n4_l = (long long)B * T * (PH / sl) * (PW / sl / 4);
  const int nbn_s = blocks_for(n4_s, NORM_BLOCKS), nbn_l = blocks_for(n4_l, NORM_BLOCKS);
  tp_normalise<<<(unsigned)(nbn_s + nbn_l), NT, 0, st>>>(w_s, region_s, n4_s, nbn_s, w_l, region_l, n4_l, (const float*)workspace, np_s, np_l);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
