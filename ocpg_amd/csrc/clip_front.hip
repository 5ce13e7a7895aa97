// Input front end of a clip: Pillow's 8-bit bilinear resize of a crop window, byte for byte, fused with the horizontal flip, ToTensor +
// Normalize and the write into the (padded) batch -- one launch per resize, no intermediate tensor in global memory.
//
// Reference: torchvision F.resize on a PIL image (datasets/transforms_video.py:211-240) is Image.resize((w, h), BILINEAR): a horizontal
// pass over the rows the vertical pass needs, then a vertical pass, EACH rounded to uint8.  Per axis the host (clip_front_func.py:
// resample_tables, fp64 as Pillow's precompute_coeffs) gives for every output index the first tap, the number of taps and the taps'
// weights as int32 = round(w * 2^22); a pass is
//     out = clip_0_255((2^21 + sum_k in[first + k] * coef[k]) >> 22)           (int32: at most 255 * (2^22 + taps / 2) + 2^21 < 2^31)
// so the device code has no floating point before the normalise step, and that step is a table look-up (mode 1: lut[(p % 3) * 256 +
// byte], the table filled by the package's own normalize_clip): the result does not depend on how a compiler treats a division.
//
// Shape: 256-thread workgroups; a workgroup owns TR output rows x 64 output columns of one plane (TR = 16, 8, 4, 2 or 1, chosen by the
// host so that the tile's source rows fit the LDS it asks for).  From the bounds of its first and last output row it knows the source
// rows y0 .. y0 + n - 1 it needs.  Pass 1: item (source row, group of 4 columns), 16 groups x 16 rows at a time, runs the horizontal
// taps from global memory (byte loads, neighbouring lanes on neighbouring bytes; the 64 columns' coefficients are re-read per row out of
// L1) and stores the 4 rounded bytes as ONE dword into the uint8 tile [n][64] in LDS -- the rounding between the passes is part of the
// result.  A half-wave's 32 stores are 2 rows x 16 consecutive dwords = 32 consecutive banks: no conflict.  Pass 2: item (output row,
// group of 4 columns) reads one dword per tap row (ds_read_b32; two output rows share a 32-lane half, so their tap rows land on the same
// 16 banks when the rows' distance is even: 2-way at worst) and accumulates the 4 columns.
// Stores: the column groups start `shift` (0..3) columns before the row so that, for a destination whose row and plane strides are
// multiples of 4 elements, every whole group is one aligned 32-bit (uint8) or 128-bit (fp32) store whatever the base offset, out_w % 4
// and the flip are; any group that is not whole or not aligned is written element by element.  Columns outside 0 .. out_w - 1 and rows
// >= out_h are never written.  Every table entry is clamped into the window / the tile before it addresses anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int TW = 64;             // output columns per workgroup
constexpr int PX = 4;              // output columns per item
constexpr int CG = TW / PX;        // column groups per tile
constexpr int RP = NT / CG;        // rows per sweep of the workgroup
constexpr int BITS = 22;           // Pillow's PRECISION_BITS
constexpr int MAX_LDS = 32768;     // bytes of dynamic LDS a launch may ask for (5 workgroups per CU by LDS)

__device__ __forceinline__ unsigned clip8(int acc) {
  const int v = acc >> BITS;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// MODE 0: uint8 destination; MODE 1: fp32 destination through the table
template <int MODE>
__global__ __launch_bounds__(NT) void clip_front(const unsigned char* __restrict__ src, long long src_plane, long long src_row, int win_h,
                                                 int win_w, const int* __restrict__ by, const int* __restrict__ ky, int ksy,
                                                 const int* __restrict__ bx, const int* __restrict__ kx, int ksx, int out_h, int out_w,
                                                 int flip, int TR, int cap, int shift, void* __restrict__ dstv, long long dst_plane,
                                                 long long dst_row, const float* __restrict__ lut) {
  extern __shared__ __align__(16) unsigned char tile[];              // [cap][TW] bytes of the horizontal pass
  const int p = blockIdx.z;
  const int r0 = blockIdx.y * TR;                                      // < out_h by the grid
  const int r1 = (r0 + TR < out_h ? r0 + TR : out_h) - 1;
  const int y0 = clampi(by[2 * r0], 0, win_h);
  const int y1 = clampi(by[2 * r1] + by[2 * r1 + 1], y0, win_h);
  const int nrows = y1 - y0 < cap ? y1 - y0 : cap;

  const int cg = threadIdx.x & (CG - 1);
  const int xb = (int)blockIdx.x * TW - shift + cg * PX;               // first output column of this thread's group, both passes

  // ---- pass 1: horizontal, global -> LDS
  {
    int xmin[PX], cnt[PX];
    const int* kc[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const int c = xb + j;
      const bool ok = c >= 0 && c < out_w;
      const int cc = ok ? c : 0;
      xmin[j] = clampi(bx[2 * cc], 0, win_w);
      int n = ok ? bx[2 * cc + 1] : 0;
      n = n < ksx ? n : ksx;
      cnt[j] = clampi(n, 0, win_w - xmin[j]);
      kc[j] = kx + (long long)cc * ksx;
    }
    const unsigned char* sp = src + (long long)p * src_plane + (long long)y0 * src_row;
    for (int row = threadIdx.x / CG; row < nrows; row += RP) {
      const unsigned char* s = sp + (long long)row * src_row;
      unsigned packed = 0u;
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        int acc = 1 << (BITS - 1);
        for (int k = 0; k < cnt[j]; ++k) acc += (int)s[xmin[j] + k] * kc[j][k];
        packed |= clip8(acc) << (8 * j);
      }
      *reinterpret_cast<unsigned*>(tile + row * TW + cg * PX) = packed;
    }
  }
  __syncthreads();

  // ---- pass 2: vertical, LDS -> destination
  const int rr = threadIdx.x / CG;
  if (rr >= TR) return;
  const int r = r0 + rr;
  if (r >= out_h || xb >= out_w || xb + PX <= 0) return;
  const int ymin = clampi(by[2 * r] - y0, 0, nrows);
  int n = by[2 * r + 1];
  n = n < ksy ? n : ksy;
  n = clampi(n, 0, nrows - ymin);
  const int* kr = ky + (long long)r * ksy;
  int acc[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) acc[j] = 1 << (BITS - 1);
  const unsigned char* t = tile + ymin * TW + cg * PX;
  for (int k = 0; k < n; ++k) {
    const unsigned w = *reinterpret_cast<const unsigned*>(t + k * TW);
    const int c = kr[k];
#pragma unroll
    for (int j = 0; j < PX; ++j) acc[j] += (int)((w >> (8 * j)) & 255u) * c;
  }
  // destination order: element d0 + i holds output column (flip ? xb + 3 - i : xb + i)
  unsigned b[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) b[i] = clip8(flip ? acc[PX - 1 - i] : acc[i]);
  const int d0 = flip ? out_w - PX - xb : xb;
  const bool whole = xb >= 0 && xb + PX <= out_w;
  const long long row_off = (long long)p * dst_plane + (long long)r * dst_row;
  if (MODE == 0) {
    unsigned char* o = reinterpret_cast<unsigned char*>(dstv) + row_off;
    if (whole && (reinterpret_cast<uintptr_t>(o + d0) & 3) == 0) {
      *reinterpret_cast<unsigned*>(o + d0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);        // little endian: element d0 is the low byte
    } else {
#pragma unroll
      for (int i = 0; i < PX; ++i)
        if (d0 + i >= 0 && d0 + i < out_w) o[d0 + i] = (unsigned char)b[i];
    }
  } else {
    const float* l = lut + (p % 3) * 256;
    float v[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) v[i] = l[b[i]];
    float* o = reinterpret_cast<float*>(dstv) + row_off;
    if (whole && (reinterpret_cast<uintptr_t>(o + d0) & 15) == 0) {
      *reinterpret_cast<float4*>(o + d0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < PX; ++i)
        if (d0 + i >= 0 && d0 + i < out_w) o[d0 + i] = v[i];
    }
  }
}

}  // namespace

extern "C" int ocpg_clip_front_u8(const unsigned char* src, int P, long long src_plane, long long src_row, int src_h, int src_w, int top,
                                  int left, int win_h, int win_w, const int* by, const int* ky, int ksy, const int* bx, const int* kx,
                                  int ksx, int out_h, int out_w, int flip, int mode, int tile_rows, int cap_rows, void* dst,
                                  long long dst_plane, long long dst_row, const float* lut, void* stream) {
  if (P <= 0 || src_h <= 0 || src_w <= 0 || win_h <= 0 || win_w <= 0 || out_h <= 0 || out_w <= 0 || ksy <= 0 || ksx <= 0) return -1006;
  if (src_plane <= 0 || src_row <= 0 || dst_plane <= 0 || dst_row <= 0) return -1006;
  if (top < 0 || left < 0 || (long long)top + win_h > src_h || (long long)left + win_w > src_w) return -2401;
  if (flip < 0 || flip > 1) return -2402;
  if (mode < 0 || mode > 1) return -2403;
  if (tile_rows != 16 && tile_rows != 8 && tile_rows != 4 && tile_rows != 2 && tile_rows != 1) return -2404;
  if (cap_rows <= 0 || (long long)cap_rows * TW > MAX_LDS) return -2405;
  if (!by || !ky || !bx || !kx) return -2406;
  if (mode == 1 && !lut) return -2407;
  if (mode == 1 && (reinterpret_cast<uintptr_t>(dst) & 3) != 0) return -2408;
  const long long gy = ((long long)out_h + tile_rows - 1) / tile_rows;
  if (gy > 65535 || P > 65535) return -1008;
  if (!src) return -1001;
  if (!dst) return -1015;
  // the column groups are laid out so that the first element a whole group stores sits on a 4-element boundary of the destination
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst) / (mode == 1 ? 4 : 1);
  const int shift = flip ? (int)((0 - (a + (uintptr_t)out_w)) & 3) : (int)(a & 3);
  const dim3 grid((unsigned)(((long long)out_w + shift + TW - 1) / TW), (unsigned)gy, (unsigned)P);
  const unsigned char* s = src + (long long)top * src_row + left;
  const size_t lds = (size_t)cap_rows * TW;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0)
    clip_front<0><<<grid, NT, lds, st>>>(s, src_plane, src_row, win_h, win_w, by, ky, ksy, bx, kx, ksx, out_h, out_w, flip, tile_rows,
                                         cap_rows, shift, dst, dst_plane, dst_row, lut);
  else
    clip_front<1><<<grid, NT, lds, st>>>(s, src_plane, src_row, win_h, win_w, by, ky, ksy, bx, kx, ksx, out_h, out_w, flip, tile_rows,
                                         cap_rows, shift, dst, dst_plane, dst_row, lut);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
