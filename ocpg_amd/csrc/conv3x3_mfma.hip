// 3x3 convolution of channels-last bf16 (or fp16: conv3x3_mfma_f16, the _h16 entry points) maps as an implicit GEMM on the matrix cores (gfx950 MFMA 32x32x16 bf16 / f16, fp32
// accumulation) -- forward and input-gradient of the 3x3 convs on the path: torchvision Bottleneck.conv2 inside the ResNet
// body (models/backbone.py:86-117), the stride-2 neck conv (models/ocpg.py:118-126), MSO's refinement convs
// (models/decoder.py:22-46).  Round 1 ran them on MIOpen: at the ResNet-101 layer3 shape (10 frames x 24 x 40, 256 -> 256
// channels, 11.3 GFLOP) its forward measured 90 us and its backward 187 us inside the step (~125 TFLOP/s, 5 % of the bf16
// MFMA peak, plus layout shuffles around its NCHW-minded solvers).
//
// GEMM view: M = N*Ho*Wo output pixels, Ngemm = Cout, K = 9*Cin ordered (ky, kx, ci) = the physical order of a
// channels-last weight [Cout, 3, 3, Cin].  No im2col buffer: the A tile of a K step (one tap, 32 input channels) is gathered
// straight from the shifted input pixels (64 contiguous bytes per row; taps outside the map read as zeros).
//   * workgroup tile 64 (pixels) x 128 (output channels), 4 waves as 2 x 2, each wave 32 x 64 = two 32x32 accumulators;
//   * K step 32: one 16-B global load per thread for A, two for B, register-prefetched one step ahead and parked in a
//     double-buffered LDS image (rows padded to 80 B: the 16 lanes of a ds_read_b128 group then hit 16 disjoint bank
//     quartets), one barrier per K step;
//   * DGRAD = true turns the same kernel into the input gradient: rows are INPUT pixels, the tap's source is the output
//     pixel (yi + 1 - ky) / stride (when divisible and inside), and the weight operand is the [Cin, 3, 3, Cout] transpose.
// The weight gradient stays a dense GEMM over the im2col matrix (csrc/im2col.hip + hipBLASLt): its K dimension is the pixel
// index, along which neither operand is contiguous.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "../../include/ocpg_hip.h"
#include "conv3x3_halo.h"
#include "h16_elem.h"

namespace {

typedef ocpg_h16::h16x8 bf16x8;
typedef ocpg_h16::f32x16 f32x16;

// The 16-bit storage type of a kernel (h16_elem.h: storage type, MFMA opcode, final narrowing -- the staging, the transposing LDS reads
// and the "bits as a signed short > 0" ReLU-mask test are type-agnostic), so the kernel has ONE body (conv3x3_mfma_kernel.h), included
// once per element type.  The bf16 kernel keeps the name and signature it had.
using ocpg_h16::Bf16;
using ocpg_h16::Fp16;

constexpr int BM = 64, BK = 64, NT = 256;        // BN (64 or 128) is a template parameter: 64 doubles the workgroups of the under-filled shapes
constexpr int LDS_ROW = BK + 8;        // bf16 elements per LDS row (144 B: 16-B aligned, rows 4 banks apart)
constexpr int SEGS = BK / 8;           // 16-B segments per staged row
constexpr int ROWS_PER_PASS = NT / SEGS;
constexpr int A_L = BM / ROWS_PER_PASS;   // 16-B loads per thread per K step (B: BN / ROWS_PER_PASS)
constexpr int NSETS = 3;               // register sets in flight

struct ConvGeom {
  int N, H, W, C;          // rows' map: output map (forward) or input map (dgrad); C = channels of the GATHERED operand
  int Hs, Ws;              // the gathered map (forward: input; dgrad: output-gradient map)
  int Cout;                // GEMM N
  int stride;
  long long M;             // N * H * W
  int ctile[3] = {0, 0, 0};      // parity-class tiles (stride-2 own-weight input gradient): first tile of classes 1, 2, 3 (class 0 starts at 0)
};

// source pixel of GEMM row (n, y, x) for tap (ky, kx); false = zero padding
template <bool DGRAD>
__device__ __forceinline__ bool tap_source(const ConvGeom& g, int y, int x, int ky, int kx, int& ys, int& xs) {
  if (!DGRAD) {
    ys = y * g.stride + ky - 1;
    xs = x * g.stride + kx - 1;
    return ys >= 0 && ys < g.Hs && xs >= 0 && xs < g.Ws;
  } else {
    const int ty = y + 1 - ky, tx = x + 1 - kx;
    if (ty < 0 || tx < 0 || (g.stride == 2 && ((ty | tx) & 1))) return false;
    ys = g.stride == 2 ? ty >> 1 : ty;
    xs = g.stride == 2 ? tx >> 1 : tx;
    return ys < g.Hs && xs < g.Ws;
  }
}

#define CONV3X3_KERNEL conv3x3_mfma
#define CONV3X3_ELEM Bf16
#include "conv3x3_mfma_kernel.h"
#undef CONV3X3_KERNEL
#undef CONV3X3_ELEM
// fp16 storage (the reference's --amp mode); instantiated for the forward, the own-weight input gradient of the shipped step and the
// neck's split-K forward
#define CONV3X3_KERNEL conv3x3_mfma_f16
#define CONV3X3_ELEM Fp16
#include "conv3x3_mfma_kernel.h"
#undef CONV3X3_KERNEL
#undef CONV3X3_ELEM

// 64-column tiles when the 128-column grid would leave the chip under-filled or badly quantised (< 3 workgroups per CU):
// layer3 of ResNet-101 at 10 frames of 384x640 is 150 x 2 = 300 workgroups on 256 CUs, layer4 38 x 4 = 152
inline bool narrow_tiles(unsigned mtiles, int ncols) {
  static const int mode = [] { const char* e = std::getenv("OCPG_CONV3X3_BN"); return e ? std::atoi(e) : 0; }();
  if (mode == 64) return true;
  if (mode == 128) return false;
  return (long long)mtiles * ((ncols + 127) / 128) < 3 * 256;
}

// A/B switch: stride-1 convolutions through the halo-staged kernel (csrc/conv3x3_halo.hip)
inline bool halo_variant() {
  static const bool on = [] { const char* e = std::getenv("OCPG_CONV3X3_HALO"); return e && e[0] == '1'; }();
  return on;
}

}  // namespace

// x [N,H,W,Cin] bf16 channels-last, w [Cout,3,3,Cin] bf16 -> y [N,Ho,Wo,Cout] bf16 = act(conv(x, w) * scale + bias); pad 1, stride 1 / 2;
// scale / bias fp32 [Cout] or NULL (1 / 0): the frozen-BN affine of the ResNet body, or a plain conv bias
// cols (may be NULL): [N*Ho*Wo, 9*Cin] bf16, the patch matrix of x in (ky, kx, ci) order = what ocpg_im2col3x3_nhwc would write
// dtype: 1 = bf16 (the very launches of ocpg_conv3x3_mfma_fwd_cols), 2 = fp16; anything else: -1010 before any launch
extern "C" int ocpg_conv3x3_mfma_fwd_cols_h16(const void* x, const void* w, const float* scale, const float* bias, int relu, int N, int H, int W,
                                              int Cin, int Cout, int stride, void* y, void* cols, int dtype, void* stream) {
  if (dtype != 1 && dtype != 2) return -1010;
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1006;
  if ((stride != 1 && stride != 2) || Cin % BK != 0) return -2000;
  if (N == 0) return 0;
  if (!x) return -1001;
  if (!w) return -1002;
  if (!y) return -1010;
  if (dtype == 1 && stride == 1 && !cols && halo_variant() &&
      ocpg_halo::conv3x3_halo((const __hip_bfloat16*)x, (const __hip_bfloat16*)w, scale, bias, relu, 0, N, H, W, Cin, Cout, (__hip_bfloat16*)y,
                              (hipStream_t)stream)) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
  }
  ConvGeom g;
  g.N = N; g.H = (H - 1) / stride + 1; g.W = (W - 1) / stride + 1; g.C = Cin; g.Hs = H; g.Ws = W; g.Cout = Cout; g.stride = stride;
  g.M = (long long)N * g.H * g.W;
  const unsigned mt = (unsigned)((g.M + BM - 1) / BM);
  const bool narrow = narrow_tiles(mt, Cout);
  const dim3 grid(mt, (unsigned)(narrow ? (Cout + 63) / 64 : (Cout + 127) / 128));
  // the patch-matrix stores are compiled in only where asked for: without them the forward fits three workgroups per CU
  const hipStream_t s = (hipStream_t)stream;
#define OCPG_FWD_LAUNCH(KERNEL, T, BN_, COLS_) \
  KERNEL<false, BN_, false, false, COLS_><<<grid, NT, 0, s>>>((const T*)x, (const T*)w, scale, bias, relu, g, (T*)y, (T*)cols)
#define OCPG_FWD_DISPATCH(KERNEL, T)                                              \
  do {                                                                            \
    if (narrow) { if (cols) OCPG_FWD_LAUNCH(KERNEL, T, 64, true); else OCPG_FWD_LAUNCH(KERNEL, T, 64, false); }   \
    else { if (cols) OCPG_FWD_LAUNCH(KERNEL, T, 128, true); else OCPG_FWD_LAUNCH(KERNEL, T, 128, false); }        \
  } while (0)
  if (dtype == 2) OCPG_FWD_DISPATCH(conv3x3_mfma_f16, __half);
  else OCPG_FWD_DISPATCH(conv3x3_mfma, __hip_bfloat16);
#undef OCPG_FWD_DISPATCH
#undef OCPG_FWD_LAUNCH
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int ocpg_conv3x3_mfma_fwd_cols(const void* x, const void* w, const float* scale, const float* bias, int relu, int N, int H, int W,
                                          int Cin, int Cout, int stride, void* y, void* cols, void* stream) {
  return ocpg_conv3x3_mfma_fwd_cols_h16(x, w, scale, bias, relu, N, H, W, Cin, Cout, stride, y, cols, 1, stream);
}

extern "C" int ocpg_conv3x3_mfma_fwd(const void* x, const void* w, const float* scale, const float* bias, int relu, int N, int H, int W,
                                     int Cin, int Cout, int stride, void* y, void* stream) {
  return ocpg_conv3x3_mfma_fwd_cols(x, w, scale, bias, relu, N, H, W, Cin, Cout, stride, y, nullptr, stream);
}

// dy [N,Ho,Wo,Cout] bf16, wT [Cin,3,3,Cout] bf16 (the weight with its channel axes swapped) -> dx [N,H,W,Cin] bf16 fully written;
// _masked: dx = conv_transpose(dy) * scale[ci] where mask_y[n,h,w,ci] > 0, else 0 (scale fp32 [Cin] or NULL = 1; mask_y like dx)
extern "C" int ocpg_conv3x3_mfma_dgrad_masked(const void* dy, const void* wT, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                              int Cout, int stride, void* dx, void* stream);
extern "C" int ocpg_conv3x3_mfma_dgrad(const void* dy, const void* wT, int N, int H, int W, int Cin, int Cout, int stride, void* dx,
                                       void* stream) {
  return ocpg_conv3x3_mfma_dgrad_masked(dy, wT, nullptr, nullptr, N, H, W, Cin, Cout, stride, dx, stream);
}

extern "C" int ocpg_conv3x3_mfma_dgrad_masked(const void* dy, const void* wT, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                              int Cout, int stride, void* dx, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1006;
  if ((stride != 1 && stride != 2) || Cout % BK != 0) return -2000;
  if (N == 0) return 0;
  if (!dy) return -1001;
  if (!wT) return -1002;
  if (!dx) return -1009;
  if (stride == 1 && !mask_y && !scale && halo_variant() &&
      ocpg_halo::conv3x3_halo((const __hip_bfloat16*)dy, (const __hip_bfloat16*)wT, nullptr, nullptr, 0, 1, N, H, W, Cout, Cin, (__hip_bfloat16*)dx,
                              (hipStream_t)stream)) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
  }
  ConvGeom g;
  g.N = N; g.H = H; g.W = W; g.C = Cout; g.Hs = (H - 1) / stride + 1; g.Ws = (W - 1) / stride + 1; g.Cout = Cin; g.stride = stride;
  g.M = (long long)N * H * W;
  const unsigned mt = (unsigned)((g.M + BM - 1) / BM);
  if (narrow_tiles(mt, Cin))
    conv3x3_mfma<true, 64><<<dim3(mt, (unsigned)((Cin + 63) / 64)), NT, 0, (hipStream_t)stream>>>(
        (const __hip_bfloat16*)dy, (const __hip_bfloat16*)wT, scale, nullptr, 0, g, (__hip_bfloat16*)dx, nullptr, (const __hip_bfloat16*)mask_y);
  else
    conv3x3_mfma<true, 128><<<dim3(mt, (unsigned)((Cin + 127) / 128)), NT, 0, (hipStream_t)stream>>>(
        (const __hip_bfloat16*)dy, (const __hip_bfloat16*)wT, scale, nullptr, 0, g, (__hip_bfloat16*)dx, nullptr, (const __hip_bfloat16*)mask_y);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

namespace {

// The input gradient from the convolution's OWN weight; classes: parity-class tiles (stride 2 only)
int dgrad_w_launch(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin, int Cout, int stride, void* dx,
                   int dtype, bool classes, void* stream) {
  if (dtype != 1 && dtype != 2) return -1010;
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1006;
  if ((stride != 1 && stride != 2) || Cout % BK != 0 || Cin % 8 != 0 || (classes && stride != 2)) return -2000;
  if (N == 0) return 0;
  if (!dy) return -1001;
  if (!w) return -1002;
  if (!dx) return -1011;
  ConvGeom g;
  g.N = N; g.H = H; g.W = W; g.C = Cout; g.Hs = (H - 1) / stride + 1; g.Ws = (W - 1) / stride + 1; g.Cout = Cin; g.stride = stride;
  g.M = (long long)N * H * W;
  unsigned mt = (unsigned)((g.M + BM - 1) / BM);
  const bool narrow = narrow_tiles(mt, Cin);      // (classes: the tile width the nine-tap launch of this shape has)
  if (classes) {      // tiles of one parity class (y & 1, x & 1) each, the heavy class first: (1,1), (0,1), (1,0), (0,0); an empty class has none
    long long t = 0;
    for (int k = 0; k < 4; ++k) {
      const int cpy = (k & 1) ^ 1, cpx = k < 2;
      t += ((long long)N * ((H - cpy + 1) / 2) * ((W - cpx + 1) / 2) + BM - 1) / BM;
      if (k < 3) g.ctile[k] = (int)t;
    }
    mt = (unsigned)t;
  }
  const dim3 grid(mt, (unsigned)(narrow ? (Cin + 63) / 64 : (Cin + 127) / 128));
  const hipStream_t s = (hipStream_t)stream;
#define OCPG_DGRAD_LAUNCH(KERNEL, T, BN_, CLS_) \
  KERNEL<true, BN_, false, true, false, CLS_><<<grid, NT, 0, s>>>((const T*)dy, (const T*)w, scale, nullptr, 0, g, (T*)dx, nullptr, (const T*)mask_y)
#define OCPG_DGRAD_DISPATCH(KERNEL, T)                                            \
  do {                                                                            \
    if (narrow) { if (classes) OCPG_DGRAD_LAUNCH(KERNEL, T, 64, true); else OCPG_DGRAD_LAUNCH(KERNEL, T, 64, false); }   \
    else { if (classes) OCPG_DGRAD_LAUNCH(KERNEL, T, 128, true); else OCPG_DGRAD_LAUNCH(KERNEL, T, 128, false); }        \
  } while (0)
  if (dtype == 2) OCPG_DGRAD_DISPATCH(conv3x3_mfma_f16, __half);
  else OCPG_DGRAD_DISPATCH(conv3x3_mfma, __hip_bfloat16);
#undef OCPG_DGRAD_DISPATCH
#undef OCPG_DGRAD_LAUNCH
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

}  // namespace

// The same from the convolution's OWN weight w [Cout, 3, 3, Cin] (no transposed copy; Cin % 8 == 0).
// dtype: 1 = bf16 (the very launches of ocpg_conv3x3_mfma_dgrad_w), 2 = fp16; anything else: -1010 before any launch
extern "C" int ocpg_conv3x3_mfma_dgrad_w_h16(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                             int Cout, int stride, void* dx, int dtype, void* stream) {
  return dgrad_w_launch(dy, w, mask_y, scale, N, H, W, Cin, Cout, stride, dx, dtype, false, stream);
}

extern "C" int ocpg_conv3x3_mfma_dgrad_w(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin, int Cout,
                                         int stride, void* dx, void* stream) {
  return ocpg_conv3x3_mfma_dgrad_w_h16(dy, w, mask_y, scale, N, H, W, Cin, Cout, stride, dx, 1, stream);
}

// The same for stride 2 (any other stride: -2000) in parity-class tiles: every tile walks only the taps that reach its pixels' class
// (9 taps per 4 pixels instead of 36); bit-identical to the nine-tap symbols for finite operands
extern "C" int ocpg_conv3x3_mfma_dgrad_w_s2_h16(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                                int Cout, int stride, void* dx, int dtype, void* stream) {
  return dgrad_w_launch(dy, w, mask_y, scale, N, H, W, Cin, Cout, stride, dx, dtype, true, stream);
}

extern "C" int ocpg_conv3x3_mfma_dgrad_w_s2(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                            int Cout, int stride, void* dx, void* stream) {
  return ocpg_conv3x3_mfma_dgrad_w_s2_h16(dy, w, mask_y, scale, N, H, W, Cin, Cout, stride, dx, 1, stream);
}

namespace {

// out[m][c] = act((sum_z part[z][m][c]) * scale[c] + bias[c]), zeroed where mask[m][c] <= 0  (out_dt 0 fp32 / 1 bf16 / 2 fp16; scale / bias / mask may
// be NULL; act = ReLU when relu != 0): the epilogues of the un-split kernel (conv bias; frozen-BN affine + ReLU; the layer in front's
// BN + ReLU backward) applied by the summing pass
__global__ __launch_bounds__(256) void k_splitk_reduce(const float* __restrict__ part, const float* __restrict__ bias, int splits, long long MC, int Cout,
                                                       void* __restrict__ out, int out_dt, const float* __restrict__ scale = nullptr, int relu = 0,
                                                       const __hip_bfloat16* __restrict__ mask = nullptr) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MC) return;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int z = 0; z < splits; ++z) {
    const float4 v = *reinterpret_cast<const float4*>(part + (long long)z * MC + i);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  const int c = (int)(i % Cout);
  if (scale) {
    const float4 sv = *reinterpret_cast<const float4*>(scale + c);
    a.x *= sv.x; a.y *= sv.y; a.z *= sv.z; a.w *= sv.w;
  }
  if (bias) {
    const float4 bv = *reinterpret_cast<const float4*>(bias + c);
    a.x += bv.x; a.y += bv.y; a.z += bv.z; a.w += bv.w;
  }
  if (relu) { a.x = fmaxf(a.x, 0.f); a.y = fmaxf(a.y, 0.f); a.z = fmaxf(a.z, 0.f); a.w = fmaxf(a.w, 0.f); }
  if (mask) {
    const ushort4 mk = *reinterpret_cast<const ushort4*>(reinterpret_cast<const unsigned short*>(mask) + i);      // bf16 > 0 <=> its bits as a signed short > 0
    if (!((short)mk.x > 0)) a.x = 0.f;
    if (!((short)mk.y > 0)) a.y = 0.f;
    if (!((short)mk.z > 0)) a.z = 0.f;
    if (!((short)mk.w > 0)) a.w = 0.f;
  }
  if (out_dt == 0) {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + i) = a;
  } else if (out_dt == 2) {
    ushort4 o;
    o.x = ocpg_h16::Fp16::bits(a.x); o.y = ocpg_h16::Fp16::bits(a.y); o.z = ocpg_h16::Fp16::bits(a.z); o.w = ocpg_h16::Fp16::bits(a.w);
    *reinterpret_cast<ushort4*>(reinterpret_cast<unsigned short*>(out) + i) = o;
  } else {
    ushort4 o;
    o.x = __bfloat16_as_ushort(__float2bfloat16(a.x)); o.y = __bfloat16_as_ushort(__float2bfloat16(a.y));
    o.z = __bfloat16_as_ushort(__float2bfloat16(a.z)); o.w = __bfloat16_as_ushort(__float2bfloat16(a.w));
    *reinterpret_cast<ushort4*>(reinterpret_cast<unsigned short*>(out) + i) = o;
  }
}

}  // namespace

// number of K ranges ocpg_conv3x3_mfma_fwd_splitk will use for this shape (a divisor of Cin / 64; 1 = the split does not pay: use the plain entry)
extern "C" int ocpg_conv3x3_mfma_splits(int N, int H, int W, int Cin, int Cout, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2) || Cin % BK != 0 || Cout % 4 != 0) return 1;
  const long long M = (long long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  const long long tiles = ((M + BM - 1) / BM) * ((Cout + 63) / 64);
  const int chunks = Cin / BK;
  int best = 1;
  for (int sgl = 1; sgl <= chunks; ++sgl)           // the largest split that keeps >= 2 chunks (18 K steps) per workgroup and <= ~1024 workgroups
    if (chunks % sgl == 0 && chunks / sgl >= 2 && tiles * sgl <= 1024) best = sgl;
  return tiles < 256 ? best : 1;
}

// part [splits][N*Ho*Wo][Cout] fp32 (scratch, fully written), y [N,Ho,Wo,Cout] = conv(x, w) + bias in out_dt (0 fp32 / dtype);
// cols as in ocpg_conv3x3_mfma_fwd_cols (may be NULL).  splits must be ocpg_conv3x3_mfma_splits(...) (> 1).
// dtype: 1 = bf16 (the very launches of ocpg_conv3x3_mfma_fwd_splitk), 2 = fp16; anything else: -1010 before any launch
extern "C" int ocpg_conv3x3_mfma_fwd_splitk_h16(const void* x, const void* w, const float* bias, int N, int H, int W, int Cin, int Cout, int stride,
                                                int splits, float* part, void* y, int out_dt, void* cols, int dtype, void* stream) {
  if (dtype != 1 && dtype != 2) return -1010;
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1006;
  if ((stride != 1 && stride != 2) || Cin % BK != 0 || Cout % 4 != 0 || splits < 1 || (Cin / BK) % splits != 0 || (out_dt != 0 && out_dt != dtype)) return -2000;
  if (N == 0) return 0;
  if (!x) return -1001;
  if (!w) return -1002;
  if (!part) return -1011;
  if (!y) return -1012;
  ConvGeom g;
  g.N = N; g.H = (H - 1) / stride + 1; g.W = (W - 1) / stride + 1; g.C = Cin; g.Hs = H; g.Ws = W; g.Cout = Cout; g.stride = stride;
  g.M = (long long)N * g.H * g.W;
  const unsigned mt = (unsigned)((g.M + BM - 1) / BM);
  const dim3 grid(mt, (unsigned)((Cout + 63) / 64), (unsigned)splits);
  if (dtype == 2 && cols)
    conv3x3_mfma_f16<false, 64, true, false, true><<<grid, NT, 0, (hipStream_t)stream>>>((const __half*)x, (const __half*)w, nullptr, nullptr, 0, g,
                                                                                       reinterpret_cast<__half*>(part), (__half*)cols);
  else if (dtype == 2)
    conv3x3_mfma_f16<false, 64, true><<<grid, NT, 0, (hipStream_t)stream>>>((const __half*)x, (const __half*)w, nullptr, nullptr, 0, g,
                                                                          reinterpret_cast<__half*>(part), nullptr);
  else if (cols)
    conv3x3_mfma<false, 64, true, false, true><<<grid, NT, 0, (hipStream_t)stream>>>(
        (const __hip_bfloat16*)x, (const __hip_bfloat16*)w, nullptr, nullptr, 0, g, reinterpret_cast<__hip_bfloat16*>(part), (__hip_bfloat16*)cols);
  else
    conv3x3_mfma<false, 64, true><<<grid, NT, 0, (hipStream_t)stream>>>(
        (const __hip_bfloat16*)x, (const __hip_bfloat16*)w, nullptr, nullptr, 0, g, reinterpret_cast<__hip_bfloat16*>(part), nullptr);
  const long long MC = g.M * Cout;
  k_splitk_reduce<<<(unsigned)((MC / 4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(part, bias, splits, MC, Cout, y, out_dt);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int ocpg_conv3x3_mfma_fwd_splitk(const void* x, const void* w, const float* bias, int N, int H, int W, int Cin, int Cout, int stride,
                                            int splits, float* part, void* y, int out_dt, void* cols, void* stream) {
  return ocpg_conv3x3_mfma_fwd_splitk_h16(x, w, bias, N, H, W, Cin, Cout, stride, splits, part, y, out_dt, cols, 1, stream);
}

// ---- split K for the ResNet body (round 4): at 2 (1) clips per step a layer3 / layer4 convolution is 300-600 (150-300) workgroups each
// walking 36-72 K steps one after the other -- a latency chain (the launch takes the SAME 45 us at 1 and at 2 clips per step).  With the
// 64-channel chunks of K split over blockIdx.z the chains are 18 steps and three times as many workgroups overlap; the summing pass
// carries the epilogue.  splits: ocpg_conv3x3_mfma_body_splits (1 = the un-split kernel is the better one).
extern "C" int ocpg_conv3x3_mfma_body_splits(long long M, int ncols, int kchannels) {
  if (M <= 0 || ncols <= 0 || kchannels <= 0 || kchannels % BK != 0 || ncols % 4 != 0) return 1;
  static const int mode = [] { const char* e = std::getenv("OCPG_CONV3X3_SPLITK"); return e ? std::atoi(e) : -1; }();       // 0: never, n > 1: force n where it divides
  const long long tiles = ((M + BM - 1) / BM) * ((ncols + 63) / 64);
  const int chunks = kchannels / BK;
  if (mode == 0) return 1;
  if (mode > 1) return chunks % mode == 0 ? mode : 1;
  if (tiles > 640) return 1;
  int best = 1;
  for (int sgl = 2; sgl <= chunks; ++sgl)
    if (chunks % sgl == 0 && chunks / sgl >= 2 && tiles * sgl <= 1280) best = sgl;
  return best;
}

// y = act(conv(x, w) * scale + shift) as in ocpg_conv3x3_mfma_fwd, K split `splits` ways; part: fp32 scratch [splits][N*Ho*Wo][Cout]
extern "C" int ocpg_conv3x3_mfma_fwd_bn_splitk(const void* x, const void* w, const float* scale, const float* shift, int relu, int N, int H, int W, int Cin,
                                               int Cout, int stride, int splits, float* part, void* y, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1006;
  if ((stride != 1 && stride != 2) || Cin % BK != 0 || Cout % 4 != 0 || splits < 2 || (Cin / BK) % splits != 0) return -2000;
  if (N == 0) return 0;
  if (!x) return -1001;
  if (!w) return -1002;
  if (!part) return -1013;
  if (!y) return -1014;
  ConvGeom g;
  g.N = N; g.H = (H - 1) / stride + 1; g.W = (W - 1) / stride + 1; g.C = Cin; g.Hs = H; g.Ws = W; g.Cout = Cout; g.stride = stride;
  g.M = (long long)N * g.H * g.W;
  const unsigned mt = (unsigned)((g.M + BM - 1) / BM);
  conv3x3_mfma<false, 64, true><<<dim3(mt, (unsigned)((Cout + 63) / 64), (unsigned)splits), NT, 0, (hipStream_t)stream>>>(
      (const __hip_bfloat16*)x, (const __hip_bfloat16*)w, nullptr, nullptr, 0, g, reinterpret_cast<__hip_bfloat16*>(part), nullptr);
  const long long MC = g.M * Cout;
  k_splitk_reduce<<<(unsigned)((MC / 4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(part, shift, splits, MC, Cout, y, 1, scale, relu);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// dx as in ocpg_conv3x3_mfma_dgrad_w (the convolution's own weight; mask_y / scale as there), K (= the output channels) split `splits` ways;
// part: fp32 scratch [splits][N*H*W][Cin]
extern "C" int ocpg_conv3x3_mfma_dgrad_w_splitk(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                                int Cout, int stride, int splits, float* part, void* dx, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1006;
  if ((stride != 1 && stride != 2) || Cout % BK != 0 || Cin % 8 != 0 || splits < 2 || (Cout / BK) % splits != 0) return -2000;
  if (N == 0) return 0;
  if (!dy) return -1001;
  if (!w) return -1002;
  if (!part) return -1012;
  if (!dx) return -1013;
  ConvGeom g;
  g.N = N; g.H = H; g.W = W; g.C = Cout; g.Hs = (H - 1) / stride + 1; g.Ws = (W - 1) / stride + 1; g.Cout = Cin; g.stride = stride;
  g.M = (long long)N * H * W;
  const unsigned mt = (unsigned)((g.M + BM - 1) / BM);
  conv3x3_mfma<true, 64, true, true><<<dim3(mt, (unsigned)((Cin + 63) / 64), (unsigned)splits), NT, 0, (hipStream_t)stream>>>(
      (const __hip_bfloat16*)dy, (const __hip_bfloat16*)w, nullptr, nullptr, 0, g, reinterpret_cast<__hip_bfloat16*>(part), nullptr);
  const long long MC = g.M * Cin;
  k_splitk_reduce<<<(unsigned)((MC / 4 + 255) / 256), 256, 0, (hipStream_t)stream>>>(part, nullptr, splits, MC, Cin, dx, 1, scale, 0, (const __hip_bfloat16*)mask_y);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
