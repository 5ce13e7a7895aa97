// A2D-Sentences / JHMDB-Sentences evaluation reduced to integer counts: per (sample, query) the three numbers from which P@K, overall
// IoU, mean IoU and the six COCO AP figures follow (reference engine.py:126-194, models/postprocessors.py:14-53, datasets/a2d_eval.py;
// the fp64 arithmetic on the counts is ocpg_amd/metrics.py: coco_ap_single_gt, RefMaskAccumulator).
//
// The reference interpolates every query's mask of the annotated frame to the original resolution, applies sigmoid, compares, inverts,
// copies Q boolean planes to the host and run-length encodes them; the evaluator decodes them again to form & and | with the ground
// truth.  Here every output pixel is decided from the [hs, ws] source (about 100 KB per plane, L2-resident) and only counted:
// nothing at the original resolution is written.
//
// Per sample b, query q and output pixel (y, x), y < out_h[b], x < out_w[b] -- the contract of ocpg_mask_tail_f32 mode 1
// (csrc/mask_tail.hip), restated:
//   virtual map  V[yy][xx] = src[b][q][yy / up][xx / up] for yy < crop_h[b], xx < crop_w[b]   (nearest replication, then the un-pad crop)
//   bilinear     ATen's align_corners=False rule in fp32, in ATen's operation order: scale = (float)crop / out;
//                s = scale * (d + 0.5f) - 0.5f, clamped at 0; i0 = (int)s; i1 = i0 + (i0 < crop - 1); l1 = s - i0; l0 = 1 - l1;
//                v = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)
//   sigmoid      p = 1 / (1 + expf(-v))
//   decision     P = p > thr, negated with `invert` (the reference's 1 - (sigmoid > 0.5); NOT v > 0, which differs for |v| < ~6e-8)
//   counts[b][q] = (|P & G|, |P|, |G|), G = the sample's ground-truth bytes != 0
//
// Shape: wave64, 256-thread workgroups = 4 rows x 64 lanes, a lane owns 4 consecutive output pixels of one row.  As in mask_tail.hip
// the groups of a row start at the 4-byte-aligned ground-truth address at or before the row's first byte, so every group wholly
// inside the row reads its four ground-truth bytes as one 32-bit load whatever out_w % 4 is; the (at most two) groups that straddle
// a row end read byte by byte.  The source indices and weights of the 4 pixels and the ground truth are formed once and reused for
// the workgroup's queries (up to 64 per workgroup; more are split over grid.z).  Each decision is counted across the wave with a
// ballot and a population count, the four waves' sums meet in LDS (plain stores to a row per wave, no LDS atomics), and the
// workgroup adds each non-zero sum to counts with ONE integer atomic.  counts is zeroed by a fill kernel first (never
// hipMemsetAsync: fill.h).  Integer arithmetic only: the result does not depend on the order of the adds.
// The grid covers the batch's largest output; workgroups beyond a sample's own out_h / out_w leave at once.  Offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"
#include "fill.h"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int ROWS = NT / 64;      // output rows per workgroup: one wave each
constexpr int PX = 4;              // output pixels per lane
constexpr int QC = 64;             // queries per workgroup
constexpr int GSLOT = 2 * QC;      // LDS slot of |G|

struct Axis {
  int i0, i1;       // source indices in the virtual map
  float l0, l1;
};

__device__ __forceinline__ Axis source_index(float scale, int d, int crop) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  int i0 = (int)s;
  i0 = i0 < crop - 1 ? i0 : crop - 1;        // never taken for d < out (s < crop - 0.5): keeps every read inside the crop regardless
  Axis a;
  a.i0 = i0;
  a.i1 = i0 + (i0 < crop - 1 ? 1 : 0);
  a.l1 = s - (float)i0;
  a.l0 = 1.f - a.l1;
  return a;
}

template <int UP>
__device__ __forceinline__ int down(int i, int up) {
  return UP == 0 ? i / up : i / UP;
}

__device__ __forceinline__ float sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

__device__ __forceinline__ int wave_count(bool b) { return __popcll(__ballot(b)); }

// UP: 1, 4, or 0 = run-time `up`
template <int UP>
__global__ __launch_bounds__(NT) void refmask_counts(const float* __restrict__ src, int Q, int hs, int ws, int up,
                                                     const int* __restrict__ geom, const unsigned char* __restrict__ gt,
                                                     const long long* __restrict__ gt_off, int qchunks, int max_out_h, int max_out_w,
                                                     float thr, int invert, int* __restrict__ counts) {
  __shared__ int part[ROWS][2 * QC + 1];
  const int b = blockIdx.z / qchunks, q0 = (blockIdx.z % qchunks) * QC;
  const int nq = Q - q0 < QC ? Q - q0 : QC;
  // the table was validated on the host before the launch; what is read here is clamped again before it addresses anything
  int crop_h = geom[4 * b + 0], crop_w = geom[4 * b + 1], out_h = geom[4 * b + 2], out_w = geom[4 * b + 3];
  crop_h = crop_h < hs * up ? crop_h : hs * up;
  crop_w = crop_w < ws * up ? crop_w : ws * up;
  out_h = out_h < max_out_h ? out_h : max_out_h;
  out_w = out_w < max_out_w ? out_w : max_out_w;
  if (crop_h <= 0 || crop_w <= 0 || out_h <= 0 || out_w <= 0) return;
  // uniform over the workgroup: nothing of it lies in this sample (a row's groups start up to 3 pixels before the row)
  if ((int)blockIdx.y * ROWS >= out_h || (long long)blockIdx.x * (64 * PX) - 3 >= out_w) return;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.y * ROWS + wave;
  const bool row_ok = y < out_h;
  const int yc = row_ok ? y : out_h - 1;
  const unsigned char* g = gt + gt_off[b] + (long long)yc * out_w;          // the row's ground truth
  const int shift = (int)(reinterpret_cast<uintptr_t>(g) & 3);
  const int x0 = (blockIdx.x * 64 + lane) * PX - shift;

  bool in[PX], gm[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    in[j] = row_ok && x0 + j >= 0 && x0 + j < out_w;
    gm[j] = false;
  }
  if (row_ok && x0 >= 0 && x0 + PX <= out_w) {
    const unsigned w = *reinterpret_cast<const unsigned*>(g + x0);          // aligned: g - shift is, and x0 + shift is a multiple of 4
#pragma unroll
    for (int j = 0; j < PX; ++j) gm[j] = ((w >> (8 * j)) & 0xffu) != 0u;     // little endian: pixel x0 is the low byte
  } else {
#pragma unroll
    for (int j = 0; j < PX; ++j)
      if (in[j]) gm[j] = g[x0 + j] != 0;
  }
  int cg = 0;
#pragma unroll
  for (int j = 0; j < PX; ++j) cg += wave_count(gm[j]);

  const float scale_y = (float)crop_h / (float)out_h, scale_x = (float)crop_w / (float)out_w;
  const Axis ay = source_index(scale_y, yc, crop_h);
  const int r0 = down<UP>(ay.i0, up), r1 = down<UP>(ay.i1, up);
  int c0[PX], c1[PX];
  float l0x[PX], l1x[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    int x = x0 + j;
    x = x < 0 ? 0 : (x < out_w ? x : out_w - 1);                     // pixels outside the row are computed on a clamped x, never counted
    const Axis ax = source_index(scale_x, x, crop_w);
    c0[j] = down<UP>(ax.i0, up);
    c1[j] = down<UP>(ax.i1, up);
    l0x[j] = ax.l0;
    l1x[j] = ax.l1;
  }

  const long long plane = (long long)hs * ws;
  for (int q = 0; q < nq; ++q) {
    const float* s = src + ((long long)b * Q + q0 + q) * plane;
    const float* s0 = s + (long long)r0 * ws;
    const float* s1 = s + (long long)r1 * ws;
    int ci = 0, cp = 0;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float a = s0[c0[j]], bb = s0[c1[j]], c = s1[c0[j]], d = s1[c1[j]];
      const float v = ay.l0 * (l0x[j] * a + l1x[j] * bb) + ay.l1 * (l0x[j] * c + l1x[j] * d);
      bool on = sigmoid(v) > thr;
      on = (invert ? !on : on) && in[j];
      cp += wave_count(on);
      ci += wave_count(on && gm[j]);
    }
    if (lane == 0) {
      part[wave][2 * q] = ci;
      part[wave][2 * q + 1] = cp;
    }
  }
  if (lane == 0) part[wave][GSLOT] = cg;
  __syncthreads();

  const int t = threadIdx.x;
  if (t < 2 * nq) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < ROWS; ++w) v += part[w][t];
    if (v) atomicAdd(&counts[((long long)b * Q + q0 + (t >> 1)) * 3 + (t & 1)], v);
  } else if (t >= GSLOT && t < GSLOT + nq) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < ROWS; ++w) v += part[w][GSLOT];
    if (v) atomicAdd(&counts[((long long)b * Q + q0 + (t - GSLOT)) * 3 + 2], v);
  }
}

static_assert(GSLOT + QC <= NT, "one thread per count");

}  // namespace

extern "C" int ocpg_refmask_counts_f32(const float* src, int B, int Q, int hs, int ws, int up, const int* geom_host, const int* geom,
                                       const unsigned char* gt, const long long* gt_off, int max_out_h, int max_out_w, float thr,
                                       int invert, int* counts, void* stream) {
  if (B <= 0 || Q <= 0 || hs <= 0 || ws <= 0 || up <= 0 || max_out_h <= 0 || max_out_w <= 0) return -1006;
  if (invert != 0 && invert != 1) return -2301;
  if (!geom_host || !geom) return -2305;
  const long long vh = (long long)hs * up, vw = (long long)ws * up;
  for (int b = 0; b < B; ++b) {
    const int* g = geom_host + 4 * (long long)b;
    if (g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] <= 0) return -1006;
    if (g[0] > vh || g[1] > vw) return -2302;
    if ((long long)g[2] * g[3] >= (1ll << 31)) return -2303;
    if (g[2] > max_out_h || g[3] > max_out_w) return -2304;
  }
  const int qchunks = (Q + QC - 1) / QC;
  const long long gy = ((long long)max_out_h + ROWS - 1) / ROWS, gz = (long long)B * qchunks;
  if (gy > 65535 || gz > 65535 || vh > 2147483647ll || vw > 2147483647ll || (long long)B * Q * 3 > 2147483647ll) return -1008;
  if (!src) return -1001;
  if (!gt || !gt_off) return -2306;
  if (!counts) return -1015;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = ocpg_fill::zero_async(counts, (size_t)B * Q * 3 * sizeof(int), st);
  if (e != hipSuccess) return -(int)e;
  // a row's groups start up to 3 pixels before the row: size grid.x for the largest shift
  const unsigned gx = (unsigned)(((long long)max_out_w + 3 + 64 * PX - 1) / (64 * PX));
  const dim3 grid(gx, (unsigned)gy, (unsigned)gz);
  if (up == 4)
    refmask_counts<4><<<grid, NT, 0, st>>>(src, Q, hs, ws, up, geom, gt, gt_off, qchunks, max_out_h, max_out_w, thr, invert, counts);
  else if (up == 1)
    refmask_counts<1><<<grid, NT, 0, st>>>(src, Q, hs, ws, up, geom, gt, gt_off, qchunks, max_out_h, max_out_w, thr, invert, counts);
  else
    refmask_counts<0><<<grid, NT, 0, st>>>(src, Q, hs, ws, up, geom, gt, gt_off, qchunks, max_out_h, max_out_w, thr, invert, counts);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
