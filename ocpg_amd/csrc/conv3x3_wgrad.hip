// Weight gradient of the 3x3 convolutions of the ResNet body (torchvision Bottleneck.conv2 inside models/backbone.py:86-117) on the matrix
// cores, straight from the two channels-last maps (round 4) -- rounds 1-3 wrote the patch (im2col) matrix [pixels, 9 Cin] (csrc/im2col.hip:
// 55 MB per layer3 convolution, 30 launches per step) and ran a row-split hipBLASLt GEMM over it.
//   gw[co][ky][kx][ci] = sum_{n, yo, xo} gz[n, yo, xo, co] * x[n, yo s + ky - 1, xo s + kx - 1, ci]          (padding 1, stride s = 1 | 2)
// GEMM view per tap: M = co, N = ci, K = output pixel.  The reduction axis is the PIXEL, along which neither operand is contiguous
// (both maps are [pixel][channel]) -- exactly the shape gfx950's transposing LDS read serves: a K chunk (a segment of <= 64 / 32 output
// pixels of one output row) is staged as it lies, Gs[pixel][64 co] and Xs[3 input rows][segment + halo][64 ci] (out-of-image rows /
// columns as zeros: that IS the padding), and both MFMA operands -- 8 consecutive pixels of one channel -- come out of
// ds_read_b64_tr_b16 (each lane supplies its own row address, so the stride-2 gather "pixel k -> column k s + kx" costs nothing).
// A workgroup owns a 64 (co) x 64 (ci) tile of ALL NINE taps (the gz fragment of a k step feeds nine MFMAs; 4 waves as 2 x 2, 9 x 16
// accumulator registers each) over a range of output rows (split K: blockIdx.z), and writes its partial tile in bf16 as
// part[z][co][9][ci] -- the layout and dtype of the row-split GEMM it replaces, so the summing stays where it was (the fused gradient
// cast, csrc/multi_cast.hip, or one ATen sum).
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "../../include/ocpg_hip.h"
#include "h16_elem.h"

namespace {

typedef ocpg_h16::h16x8 bf16x8;
typedef short s4 __attribute__((ext_vector_type(4)));
typedef ocpg_h16::f32x16 f32x16;
using ocpg_h16::Bf16;      // storage type of a kernel (h16_elem.h): the MFMA opcode and the narrowing of the partial sums are all that differ
using ocpg_h16::Fp16;

constexpr int NT = 256, TM = 64, TN = 64, LROW = 72;       // tile edges (channels), LDS row in bf16 elements (144 B: 16-byte aligned)

// fragment: 8 consecutive k (rows r0 + 8 fh + 0..7 at row pitch `pitch` LDS rows) of column c0 + (lane & 31) of a [row][LROW] tile
__device__ __forceinline__ bf16x8 tr_frag(const short* tile, int r0, int pitch, int c0, int lane) {
  const int li = lane & 15, grp = lane >> 4, fh = lane >> 5;
  const short* p = tile + (r0 + (8 * fh + (li >> 2)) * pitch) * LROW + c0 + 16 * (grp & 1) + 4 * (li & 3);
  const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
  const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(p + 4 * pitch * LROW));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3]; r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// v or zeros, component by component (a select between two uint4 OBJECTS is lowered through their addresses and drags both into scratch)
__device__ __forceinline__ uint4 keep(uint4 v, bool yes) { return make_uint4(yes ? v.x : 0u, yes ? v.y : 0u, yes ? v.z : 0u, yes ? v.w : 0u); }

struct WG {
  int N, H, W, Ho, Wo, Cin, Cout, stride, seg, xw, rows_per_split;
};

#define WGRAD_KERNEL conv3x3_wgrad
#define WGRAD_ELEM Bf16
#include "conv3x3_wgrad_kernel.h"
#undef WGRAD_KERNEL
#undef WGRAD_ELEM
#define WGRAD_KERNEL conv3x3_wgrad_f16
#define WGRAD_ELEM Fp16
#include "conv3x3_wgrad_kernel.h"
#undef WGRAD_KERNEL
#undef WGRAD_ELEM

inline int seg_of(int stride) { return stride == 1 ? 64 : 32; }

// ---- the ring kernel (conv3x3_wgrad_ring_kernel.h): rolling input rows, one barrier per step, 8 waves with the taps split 5 + 4
constexpr int NTR = 512;
template <int V>
struct IC { static constexpr int value = V; };

#define WGRAD_RING_KERNEL conv3x3_wgrad_ring
#define WGRAD_ELEM Bf16
#include "conv3x3_wgrad_ring_kernel.h"
#undef WGRAD_RING_KERNEL
#undef WGRAD_ELEM
#define WGRAD_RING_KERNEL conv3x3_wgrad_ring_f16
#define WGRAD_ELEM Fp16
#include "conv3x3_wgrad_ring_kernel.h"
#undef WGRAD_RING_KERNEL
#undef WGRAD_ELEM

}  // namespace

extern "C" {

/* number of row ranges (the leading dimension of `part`) ocpg_conv3x3_mfma_wgrad uses for this shape: one workgroup per CU (every extra
 * range is another [Cout, 9 Cin] partial for the summing pass to read) */
int ocpg_conv3x3_mfma_wgrad_splits(int N, int H, int W, int Cin, int Cout, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2)) return 0;
  const long long rows = (long long)N * ((H - 1) / stride + 1);
  const long long tiles = (long long)((Cout + TM - 1) / TM) * ((Cin + TN - 1) / TN);
  static const int target = [] { const char* e = std::getenv("OCPG_WGRAD_WGS"); return e && *e ? std::atoi(e) : 256; }();
  long long s = (target + tiles - 1) / tiles;
  if (s > rows) s = rows;
  if (s < 1) s = 1;
  const long long rps = (rows + s - 1) / s;
  return (int)((rows + rps - 1) / rps);
}

/* dtype: 1 = bf16 (the very launches of ocpg_conv3x3_mfma_wgrad), 2 = fp16 (part in fp16 too); anything else: -1010 before any launch */
int ocpg_conv3x3_mfma_wgrad_h16(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, int dtype,
                                void* stream) {
  if (dtype != 1 && dtype != 2) return -1010;
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1003;
  if ((stride != 1 && stride != 2) || Cin % 8 != 0 || Cout % 8 != 0) return -2000;
  if (N == 0) return 0;
  if (!gz) return -1001;
  if (!x) return -1002;
  if (!part) return -1009;
  WG g;
  g.N = N; g.H = H; g.W = W; g.Ho = (H - 1) / stride + 1; g.Wo = (W - 1) / stride + 1; g.Cin = Cin; g.Cout = Cout; g.stride = stride;
  g.seg = seg_of(stride);
  g.xw = (g.seg - 1) * stride + 3;
  const int splits = ocpg_conv3x3_mfma_wgrad_splits(N, H, W, Cin, Cout, stride);
  const long long rows = (long long)N * g.Ho;
  g.rows_per_split = (int)((rows + splits - 1) / splits);
  const dim3 grid((unsigned)((Cout + TM - 1) / TM), (unsigned)((Cin + TN - 1) / TN), (unsigned)splits);
  if (dtype == 2) {
    if (stride == 1) conv3x3_wgrad_f16<1, 64><<<grid, NT, 0, (hipStream_t)stream>>>((const __half*)gz, (const __half*)x, g, (__half*)part);
    else conv3x3_wgrad_f16<2, 32><<<grid, NT, 0, (hipStream_t)stream>>>((const __half*)gz, (const __half*)x, g, (__half*)part);
  } else if (stride == 1) {
    conv3x3_wgrad<1, 64><<<grid, NT, 0, (hipStream_t)stream>>>((const __hip_bfloat16*)gz, (const __hip_bfloat16*)x, g, (__hip_bfloat16*)part);
  } else {
    conv3x3_wgrad<2, 32><<<grid, NT, 0, (hipStream_t)stream>>>((const __hip_bfloat16*)gz, (const __hip_bfloat16*)x, g, (__hip_bfloat16*)part);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

int ocpg_conv3x3_mfma_wgrad(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, void* stream) {
  return ocpg_conv3x3_mfma_wgrad_h16(gz, x, N, H, W, Cin, Cout, stride, part, 1, stream);
}

/* The ring kernel on the same operands: same validation order, return codes, `part` layout and split as ocpg_conv3x3_mfma_wgrad_h16, and
 * bit-identical partial sums.  It serves maps of one segment per output row (Wo <= 64 under stride 1, <= 32 under stride 2); a wider map
 * is declined with -2000 before any launch, and the caller runs the kernel above. */
int ocpg_conv3x3_mfma_wgrad_ring_h16(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, int dtype,
                                     void* stream) {
  if (dtype != 1 && dtype != 2) return -1010;
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return -1003;
  if ((stride != 1 && stride != 2) || Cin % 8 != 0 || Cout % 8 != 0) return -2000;
  if ((W - 1) / stride + 1 > seg_of(stride)) return -2000;
  if ((long long)W * Cin > 0x7fffffffLL || (long long)W * Cout > 0x7fffffffLL) return -2000;      // offsets inside a map row are ints
  if (N == 0) return 0;
  if (!gz) return -1001;
  if (!x) return -1002;
  if (!part) return -1009;
  WG g;
  g.N = N; g.H = H; g.W = W; g.Ho = (H - 1) / stride + 1; g.Wo = (W - 1) / stride + 1; g.Cin = Cin; g.Cout = Cout; g.stride = stride;
  g.seg = seg_of(stride);
  g.xw = (g.seg - 1) * stride + 3;
  const int splits = ocpg_conv3x3_mfma_wgrad_splits(N, H, W, Cin, Cout, stride);
  const long long rows = (long long)N * g.Ho;
  g.rows_per_split = (int)((rows + splits - 1) / splits);
  const dim3 grid((unsigned)((Cout + TM - 1) / TM), (unsigned)((Cin + TN - 1) / TN), (unsigned)splits);
  const hipStream_t st = (hipStream_t)stream;
  const int ks = (g.Wo + 15) / 16;      // k steps per output row: 1..4 under stride 1, 1..2 under stride 2
#define RING(S_, SEG_, KS_)                                                                                                  \
  if (dtype == 2) conv3x3_wgrad_ring_f16<S_, SEG_, KS_><<<grid, NTR, 0, st>>>((const __half*)gz, (const __half*)x, g, (__half*)part); \
  else conv3x3_wgrad_ring<S_, SEG_, KS_><<<grid, NTR, 0, st>>>((const __hip_bfloat16*)gz, (const __hip_bfloat16*)x, g, (__hip_bfloat16*)part)
  if (stride == 1) {
    if (ks == 1) { RING(1, 64, 1); } else if (ks == 2) { RING(1, 64, 2); } else if (ks == 3) { RING(1, 64, 3); } else { RING(1, 64, 4); }
  } else {
    if (ks == 1) { RING(2, 32, 1); } else { RING(2, 32, 2); }
  }
#undef RING
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

int ocpg_conv3x3_mfma_wgrad_ring(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, void* stream) {
  return ocpg_conv3x3_mfma_wgrad_ring_h16(gz, x, N, H, W, Cin, Cout, stride, part, 1, stream);
}

}  // extern "C"
