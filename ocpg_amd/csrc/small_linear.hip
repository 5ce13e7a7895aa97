// Linear layers over FEW rows (the decoder: 50 query rows; heads, controller, LFM coefficient MLPs: 10..200 rows) in one launch
// forward and ONE launch backward.
//
// Reference: every nn.Linear of the decoder layers, the box / class heads and the controller (models/deformable_transformer.py:
// 313-336, models/ocpg.py:83-110,325-349).  Under autocast each of them is a cast of the input + addmm forward and two mm + a bias
// reduction + a cast of the input gradient backward: 6 launches whose work is a few MFLOP -- on MI355X a graph kernel node costs
// ~5 us of GPU timeline even when empty, so the step pays the launches, not the math (~50 such layers per step).
//   forward :  y[r, co]  = sum_ci x[r, ci] w[co, ci] + b[co]                      (x fp32 or h16, w / b / y h16)
//   backward:  gx[r, ci] = sum_co gy[r, co] w[co, ci]                             (gx in x's dtype)
//              gw[co, ci] = sum_r gy[r, co] x[r, ci],   gb[co] = sum_r gy[r, co]   (h16, like autograd's gradients of 16-bit copies)
// h16 = the autocast dtype: bf16 (sl_fwd / sl_bwd) or fp16 (sl_fwd_f16 / sl_bwd_f16, the reference's --amp mode; the _h16 entry points
// with dtype 2) -- ONE kernel body (small_linear_kernel.h) included once per element trait.  An fp32 x / gy is rounded to the storage type
// to nearest-even while it is staged; in fp16 a value past 65504 becomes inf as ATen's cast makes it (no clamping: the GradScaler deals
// with it).  All arithmetic is fp32.
// 64 x 64 x 64 tiles of v_mfma_f32_32x32x16_bf16 / _f16, 4 waves (2 x 2); operands whose reduction axis is not contiguous in memory
// (w for gx; gy and x for gw) are transposed while they are staged into LDS.  Cin must be a multiple of 64; anything else returns
// -2000 and the caller keeps the library path.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"
#include "h16_elem.h"

namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int T = 64, LROW = T + 8, NT = 256;      // tile edge, LDS row (144 B), threads

// The element trait of a kernel: h16_elem.h's storage type, MFMA opcode and RNE narrowing + what this file needs on top: the bits of a
// narrowed value as the `short` the staging code moves (f2b) and the widening to fp32 (b2f).  Elements travel as bits; every function
// below that looks at a VALUE takes the trait.
struct Bf16 : ocpg_h16::Bf16 {
  static __device__ __forceinline__ short f2b(float v) { return (short)__bfloat16_as_ushort(__float2bfloat16(v)); }
  static __device__ __forceinline__ float widen(short b) { return __uint_as_float(((unsigned)(unsigned short)b) << 16); }
};
struct Fp16 : ocpg_h16::Fp16 {
  static __device__ __forceinline__ short f2b(float v) { return (short)bits(v); }      // RNE; past 65504: inf, NaN stays NaN
  static __device__ __forceinline__ float widen(short b) { return __half2float(__ushort_as_half((unsigned short)b)); }
};

// element (row, col) of a [rows, cols] matrix stored as fp32 (is_f32) or in the 16-bit type, 0 outside
template <typename E>
__device__ __forceinline__ short ld_el(const void* p, int is_f32, long long ld, int row, int col, int rows, int cols) {
  if (row >= rows || col >= cols) return 0;
  return is_f32 ? E::f2b(reinterpret_cast<const float*>(p)[row * ld + col]) : reinterpret_cast<const short*>(p)[row * ld + col];
}

// 16 consecutive elements of row `row` starting at column `col` (fp32 or 16-bit storage) as 16-bit bits, zeros outside the matrix;
// 16-byte loads when the run is inside and aligned
template <typename E>
__device__ __forceinline__ void ld16_raw(short (&v)[16], const void* p, int is_f32, long long ld, int row, int col, int rows, int cols) {
  if (row < rows && col + 16 <= cols && ((ld | col) & 7) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {     // (a view with a storage offset may be unaligned)
    if (is_f32) {
      const float4* q = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + row * ld + col);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 f = q[u];
        v[4 * u] = E::f2b(f.x); v[4 * u + 1] = E::f2b(f.y); v[4 * u + 2] = E::f2b(f.z); v[4 * u + 3] = E::f2b(f.w);
      }
    } else {
      const bf16x8* q = reinterpret_cast<const bf16x8*>(reinterpret_cast<const short*>(p) + row * ld + col);
      const bf16x8 a = q[0], b = q[1];
#pragma unroll
      for (int u = 0; u < 8; ++u) { v[u] = a[u]; v[8 + u] = b[u]; }
    }
  } else {
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = ld_el<E>(p, is_f32, ld, row, col + u, rows, cols);
  }
}

// the same with an optional ReLU mask: `mask` = the 16-bit output y of a fused ReLU (same shape as p): gy is zeroed where y <= 0
template <typename E>
__device__ __forceinline__ void ld16(short (&v)[16], const void* p, int is_f32, long long ld, int row, int col, int rows, int cols,
                                     const short* mask = nullptr) {
  ld16_raw<E>(v, p, is_f32, ld, row, col, rows, cols);
  if (mask) {
    short m[16];
    ld16_raw<E>(m, mask, 0, ld, row, col, rows, cols);
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = E::widen(m[u]) > 0.f ? v[u] : (short)0;
  }
}

// A thread's share of one staged T x T tile: 16 consecutive elements of tile row threadIdx.x >> 2 (as 16-bit bits)
struct Seg {
  bf16x8 a, b;
};

template <typename E>
__device__ __forceinline__ Seg load_seg(const void* src, int is_f32, long long ld, int r0, int c0, int rows, int cols, const short* mask = nullptr) {
  const int row = threadIdx.x >> 2, seg = threadIdx.x & 3;
  short v[16];
  ld16<E>(v, src, is_f32, ld, r0 + row, c0 + seg * 16, rows, cols, mask);
  Seg s;
#pragma unroll
  for (int u = 0; u < 8; ++u) { s.a[u] = v[u]; s.b[u] = v[8 + u]; }
  return s;
}

// park it as [tile row][tile col] (reduction axis = columns of the source)
__device__ __forceinline__ void commit_plain(short* dst, const Seg& s) {
  const int row = threadIdx.x >> 2, seg = threadIdx.x & 3;
  *reinterpret_cast<bf16x8*>(dst + row * LROW + seg * 16) = s.a;
  *reinterpret_cast<bf16x8*>(dst + row * LROW + seg * 16 + 8) = s.b;
}

// park it TRANSPOSED: LDS [tile col][tile row] (reduction axis = rows of the source)
__device__ __forceinline__ void commit_transposed(short* dst, const Seg& s) {
  const int row = threadIdx.x >> 2, seg = threadIdx.x & 3;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    dst[(seg * 16 + u) * LROW + row] = s.a[u];
    dst[(seg * 16 + 8 + u) * LROW + row] = s.b[u];
  }
}

// one K step (64) of the 64 x 64 tile product: wave (wm, wn) owns the 32 x 32 block
template <typename E>
__device__ __forceinline__ f32x16 tile_mma(const short* As, const short* Bs, f32x16 acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave & 1, wn = wave >> 1, fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int kk = 0; kk < T / 16; ++kk) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(As + (wm * 32 + fr) * LROW + kk * 16 + fh * 8);
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (wn * 32 + fr) * LROW + kk * 16 + fh * 8);
    acc = E::mfma(a, b, acc);
  }
  return acc;
}

// The K loop: the global loads of PF consecutive K steps are issued back to back, then the steps are parked and multiplied one by
// one -- these launches are a chain of (load latency -> barrier -> 4 MFMAs) per step and nothing else runs on the CU, so the latency
// is paid once per PF steps instead of once per step (Cin = 256: 1 instead of 4; the FFN's 1024: 4 instead of 16).
constexpr int PF = 4;
template <typename E, bool TA, bool TB, typename LA, typename LB>
__device__ __forceinline__ f32x16 k_loop(int nk, short* As, short* Bs, LA load_a, LB load_b, f32x16 acc) {
  for (int kb = 0; kb < nk; kb += PF) {
    Seg sa[PF], sb[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j)
      if (kb + j < nk) { sa[j] = load_a((kb + j) * T); sb[j] = load_b((kb + j) * T); }
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      if (kb + j < nk) {
        if (TA) commit_transposed(As, sa[j]); else commit_plain(As, sa[j]);
        if (TB) commit_transposed(Bs, sb[j]); else commit_plain(Bs, sb[j]);
        __syncthreads();
        acc = tile_mma<E>(As, Bs, acc);
        __syncthreads();
      }
    }
  }
  return acc;
}

// store the wave's 32 x 32 block of C[m0.., n0..] (row-major [M, N], fp32 or the 16-bit type), + optional per-column bias
template <typename E>
__device__ __forceinline__ void store_tile(void* C, int out_f32, long long ld, int m0, int n0, int M, int N, f32x16 acc, const short* bias,
                                           int relu = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave & 1, wn = wave >> 1;
  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= N) return;
  const float bv = bias ? E::widen(bias[col]) : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (row < M) {
      float v = acc[i] + bv;
      if (relu) v = fmaxf(v, 0.f);
      if (out_f32) reinterpret_cast<float*>(C)[row * ld + col] = v;
      else reinterpret_cast<short*>(C)[row * ld + col] = E::f2b(v);
    }
  }
}

#define SL_FWD sl_fwd
#define SL_BWD sl_bwd
#define SL_ELEM Bf16
#include "small_linear_kernel.h"
#undef SL_FWD
#undef SL_BWD
#undef SL_ELEM
// fp16 storage (the reference's --amp mode)
#define SL_FWD sl_fwd_f16
#define SL_BWD sl_bwd_f16
#define SL_ELEM Fp16
#include "small_linear_kernel.h"
#undef SL_FWD
#undef SL_BWD
#undef SL_ELEM

inline int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

}  // namespace

extern "C" {

/* y [R, Cout] h16 = act(x [R, Cin] (fp32: x_f32 != 0, else h16) . w[Cout, Cin]^T (h16) + b [Cout] (h16 or NULL)), act = ReLU when
 * relu != 0.  dtype: 1 = bf16 (the very launch of ocpg_small_linear_fwd), 2 = fp16; anything else: -1010 before any other check.
 * -2000: not served. */
int ocpg_small_linear_fwd_h16(const void* x, int x_f32, const void* w, const void* b, int R, int Cin, int Cout, int relu, void* y, int dtype,
                              void* stream) {
  if (dtype != 1 && dtype != 2) return -1010;
  if (R < 0 || Cin <= 0 || Cout <= 0) return -1005;
  if (Cin % T != 0 || R > 4096) return -2000;
  if (R == 0) return 0;
  if (!x) return -1001;
  if (!w) return -1003;
  if (!y) return -1008;
  const dim3 grid((Cout + T - 1) / T, (R + T - 1) / T);
  if (dtype == 2)
    sl_fwd_f16<<<grid, NT, 0, (hipStream_t)stream>>>(x, x_f32, (const short*)w, (const short*)b, R, Cin, Cout, relu, (short*)y);
  else
    sl_fwd<<<grid, NT, 0, (hipStream_t)stream>>>(x, x_f32, (const short*)w, (const short*)b, R, Cin, Cout, relu, (short*)y);
  return status();
}

int ocpg_small_linear_fwd(const void* x, int x_f32, const void* w, const void* b, int R, int Cin, int Cout, int relu, void* y, void* stream) {
  return ocpg_small_linear_fwd_h16(x, x_f32, w, b, R, Cin, Cout, relu, y, 1, stream);
}

/* gx [R, Cin] (x's dtype; NULL: not needed), gw [Cout, Cin] h16, gb [Cout] h16 (NULL: no bias) from gy [R, Cout] (fp32 / h16);
 * y_relu = the forward's output when it applied the ReLU (gy is masked where y <= 0), else NULL.  dtype as above. */
int ocpg_small_linear_bwd_h16(const void* gy, int gy_f32, const void* x, int x_f32, const void* w, const void* y_relu, int R, int Cin, int Cout,
                              void* gx, void* gw, void* gb, int dtype, void* stream) {
  if (dtype != 1 && dtype != 2) return -1010;
  if (R < 0 || Cin <= 0 || Cout <= 0) return -1006;
  if (Cin % T != 0 || R > 4096) return -2000;
  if (!gy) return -1001;
  if (!x) return -1003;
  if (!w) return -1005;
  if (!gw) return -1010;
  const int n_dx = gx ? ((R + T - 1) / T) * ((Cin + T - 1) / T) : 0;
  const int n_dw = ((Cout + T - 1) / T) * ((Cin + T - 1) / T);
  if (dtype == 2)
    sl_bwd_f16<<<n_dx + n_dw, NT, 0, (hipStream_t)stream>>>(gy, gy_f32, x, x_f32, (const short*)w, (const short*)y_relu, R, Cin, Cout, n_dx,
                                                            gx != nullptr, gx, (short*)gw, (short*)gb);
  else
    sl_bwd<<<n_dx + n_dw, NT, 0, (hipStream_t)stream>>>(gy, gy_f32, x, x_f32, (const short*)w, (const short*)y_relu, R, Cin, Cout, n_dx,
                                                        gx != nullptr, gx, (short*)gw, (short*)gb);
  return status();
}

int ocpg_small_linear_bwd(const void* gy, int gy_f32, const void* x, int x_f32, const void* w, const void* y_relu, int R, int Cin, int Cout,
                          void* gx, void* gw, void* gb, void* stream) {
  return ocpg_small_linear_bwd_h16(gy, gy_f32, x, x_f32, w, y_relu, R, Cin, Cout, gx, gw, gb, 1, stream);
}

}  // extern "C"
