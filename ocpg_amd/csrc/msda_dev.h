// Device helpers shared by the MSDeformAttn kernels (row kernels in msda.hip, column-tile kernels in msda_col.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ocpg_dev {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---- 16-bit STORAGE of value / out / grad_out (the _h16 entry points; arithmetic stays fp32) ---------------------------
// Tag types: a pointer's element type picks the conversion, so a kernel templated on its grad_out type keeps `ld4(p)` /
// `ld1(p)` at its one load site and the float instantiation compiles to what it was.
struct bf16s { unsigned short bits; };
struct fp16s { unsigned short bits; };
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16s* p) { return __uint_as_float((unsigned)p->bits << 16); }
__device__ __forceinline__ float ld1(const fp16s* p) { return (float)*reinterpret_cast<const _Float16*>(p); }

__device__ __forceinline__ float2 cvt2(unsigned u, const bf16s*) { return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)); }
__device__ __forceinline__ float2 cvt2(unsigned u, const fp16s*) {
  const half2v h = __builtin_bit_cast(half2v, u);
  return make_float2((float)h.x, (float)h.y);
}
// four channels = one 8-byte load
__device__ __forceinline__ float4 ld4(const bf16s* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  const float2 a = cvt2(u.x, p), b = cvt2(u.y, p);
  return make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ float4 ld4(const fp16s* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  const float2 a = cvt2(u.x, p), b = cvt2(u.y, p);
  return make_float4(a.x, a.y, b.x, b.y);
}
// CPL channels per lane: 4 (8-byte load) or 8 (16-byte load)
template <int CPL, typename H>
__device__ __forceinline__ void ldc(const H* p, float (&f)[CPL]) {
  if constexpr (CPL == 4) {
    const float4 v = ld4(p);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
    static_assert(CPL == 8, "4 or 8 channels per lane");
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const float2 a = cvt2(u.x, p), b = cvt2(u.y, p), c = cvt2(u.z, p), d = cvt2(u.w, p);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
  }
}
// The same in two steps, for corners that may lie outside the map: the raw bits are ALWAYS fetched (from a safe address when the corner is
// outside), ANDed with an all-ones / all-zeros word (zero bits widen to 0.0f in both formats; exact whatever the safe address holds) and
// widened after all loads of a sample have been issued.  A load + widening under a condition put a wait for the memory behind every
// single load -- four serial round trips per sample instead of one (measured: +30 % on the forward) -- and
// whether the optimiser keeps a widening out of the load's branch turned out to depend on the format and the lane mapping.
template <int CPL> struct RawC { typedef uint2 type; };
template <> struct RawC<8> { typedef uint4 type; };
template <int CPL, typename H>
__device__ __forceinline__ typename RawC<CPL>::type ldraw(const H* p) { return *reinterpret_cast<const typename RawC<CPL>::type*>(p); }
__device__ __forceinline__ uint2 keep(const uint2 r, unsigned m) { return make_uint2(r.x & m, r.y & m); }
__device__ __forceinline__ uint4 keep(const uint4 r, unsigned m) { return make_uint4(r.x & m, r.y & m, r.z & m, r.w & m); }
template <typename H>
__device__ __forceinline__ void widen(const uint2 u, const H* tag, float (&f)[4]) {
  const float2 a = cvt2(u.x, tag), b = cvt2(u.y, tag);
  f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
}
template <typename H>
__device__ __forceinline__ void widen(const uint4 u, const H* tag, float (&f)[8]) {
  const float2 a = cvt2(u.x, tag), b = cvt2(u.y, tag), c = cvt2(u.z, tag), d = cvt2(u.w, tag);
  f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
}
// one round-to-nearest-even per stored element (NaN stays NaN)
__device__ __forceinline__ unsigned short rne16(float f, const bf16s*) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ unsigned short rne16(float f, const fp16s*) {
  const _Float16 h = (_Float16)f;          // v_cvt_f16_f32, round mode of the kernel = nearest even
  return __builtin_bit_cast(unsigned short, h);
}
template <typename H>
__device__ __forceinline__ void st1(H* p, float f) { p->bits = rne16(f, p); }
template <int CPL, typename H>
__device__ __forceinline__ void stc(H* p, const float (&f)[CPL]) {
  unsigned w[CPL / 2];
#pragma unroll
  for (int i = 0; i < CPL / 2; ++i) w[i] = (unsigned)rne16(f[2 * i], p) | ((unsigned)rne16(f[2 * i + 1], p) << 16);
  if constexpr (CPL == 4) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  else *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- cross-lane sums inside an 8-lane row group without touching LDS (DPP) ---------------------------------
__device__ __forceinline__ float dpp_xor1(float v) {   // quad_perm [1,0,3,2]
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_xor2(float v) {   // quad_perm [2,3,0,1]
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_mirror8(float v) {   // row_half_mirror: lane i <-> 7-i inside each 8-lane group
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));
}

// Sum 4 samples x {ga, gx, gy} over the 8 lanes of a row as a reduce-scatter: after it, the lane pair
// (j>>1) == s holds sample s's three totals (12 DPP moves instead of 36 LDS-crossbar shuffles).
// v[s][c] in; returns this lane's sample index, totals in out[0..2].
__device__ __forceinline__ int reduce_scatter_g8_p4(const float (&v)[4][3], int j, float (&out)[3]) {
  const bool hi = (j & 4) != 0;          // step 1: partner 7-j (opposite bit 2); keep samples {0,1} (low half) or {2,3}
  float a[2][3];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float keep = hi ? v[2 + s][c] : v[s][c];
      const float send = hi ? v[s][c] : v[2 + s][c];
      a[s][c] = keep + dpp_mirror8(send);
    }
  const bool mid = (j & 2) != 0;         // step 2: partner j^2; keep sample 0 or 1 of the pair
  float b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float keep = mid ? a[1][c] : a[0][c];
    const float send = mid ? a[0][c] : a[1][c];
    b[c] = keep + dpp_xor2(send);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = b[c] + dpp_xor1(b[c]);   // step 3: all-reduce over the last pair
  return (hi ? 2 : 0) + (mid ? 1 : 0);
}

// ---- per-sample records of the row kernels (fp32: msda.hip, 16-bit storage: msda_h16.hip) --------------------------------
// One precomputed sample, 32 bytes = two ds_read_b128.
struct __attribute__((aligned(16))) SampleRec {
  int off00;      // element offset (in scalars, relative to value[b, 0, m, 0]) of corner (y0, x0); may be "virtual" (negative) when that corner is outside
  int rowstride;  // W * M * D
  int mask;       // bit k set <=> corner k (0:(y0,x0) 1:(y0,x1) 2:(y1,x0) 3:(y1,x1)) is inside the map; 0 => sample skipped
  float a;        // attention weight
  float ly, lx;   // fractional parts
  float H, W;     // level size as float (grad_loc scaling)
};

template <typename T>
__device__ __forceinline__ void make_sample(T x_n, T y_n, T a, int H, int W, int lstart, int MD, SampleRec& r) {
  const T h_im = y_n * (T)H - (T)0.5;
  const T w_im = x_n * (T)W - (T)0.5;
  r.a = (float)a;
  r.H = (float)H;
  r.W = (float)W;
  r.rowstride = W * MD;
  if (h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W) {
    const int y0 = (int)floor(h_im), x0 = (int)floor(w_im);
    r.ly = (float)(h_im - (T)y0);
    r.lx = (float)(w_im - (T)x0);
    const bool y0ok = y0 >= 0, y1ok = y0 + 1 <= H - 1, x0ok = x0 >= 0, x1ok = x0 + 1 <= W - 1;
    r.mask = (y0ok && x0ok ? 1 : 0) | (y0ok && x1ok ? 2 : 0) | (y1ok && x0ok ? 4 : 0) | (y1ok && x1ok ? 8 : 0);
    r.off00 = (lstart + y0 * W + x0) * MD;
  } else {
    r.ly = r.lx = 0.f;
    r.mask = 0;
    r.off00 = 0;
  }
}

struct __attribute__((aligned(16))) GatherRec {
  int pk;          // element offset of corner (ya, xa) relative to value[b, 0, m, 0]  |  iy1<<3 | iy0<<2 | ix1<<1 | ix0
  int rowstride;   // W * M * D
  float aW, aH;    // attention weight * level width / height (grad_loc scaling)
  float hy, ly, hx, lx;   // masked by validity
};

// record of the gather row kernels (msda_bwd_gather_row, msda_bwd_gather_h16): validity folded into the per-axis weights, the corner
// address clamped into the map
__device__ __forceinline__ void make_gather(float x_n, float y_n, float a, int H, int W, int lstart, int MD, GatherRec& rec) {
  const float h_im = y_n * (float)H - 0.5f, w_im = x_n * (float)W - 0.5f;
  rec.rowstride = W * MD;
  if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
    const int y0 = (int)floorf(h_im), x0 = (int)floorf(w_im);
    const float ly = h_im - (float)y0, lx = w_im - (float)x0;
    const bool iy0 = y0 >= 0, iy1 = y0 + 1 <= H - 1, ix0 = x0 >= 0, ix1 = x0 + 1 <= W - 1;
    rec.hy = iy0 ? 1.f - ly : 0.f;
    rec.ly = iy1 ? ly : 0.f;
    rec.hx = ix0 ? 1.f - lx : 0.f;
    rec.lx = ix1 ? lx : 0.f;
    rec.aW = a * (float)W;
    rec.aH = a * (float)H;
    rec.pk = ((lstart + max(y0, 0) * W + max(x0, 0)) * MD) | (iy1 ? 8 : 0) | (iy0 ? 4 : 0) | (ix1 ? 2 : 0) | (ix0 ? 1 : 0);
  } else {
    rec.hy = rec.ly = rec.hx = rec.lx = rec.aW = rec.aH = 0.f;
    rec.pk = 0;
  }
}

}  // namespace ocpg_dev
