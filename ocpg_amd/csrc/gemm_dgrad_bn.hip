// Input gradient of a 1x1 convolution of the ResNet body WITH the frozen-BN + ReLU backward of the layer in front in its epilogue
// (gfx950 MFMA 32x32x16 bf16 or f16, fp32 accumulation).  Until now each such site was a hipBLASLt GEMM (no ReLU-mask epilogue there)
// followed by a pure memory pass, ocpg_bn_act_bwd (csrc/bn_act.hip): 57 of its 63 launches per step sat right behind one of these GEMMs.
//
// GEMM view (channels-last maps, the 1x1 weight as it lies):
//   v[m, n] = sum_k A[m, k] W[k, n]      A = the output gradient after this convolution's own BN backward [M, K] (K contiguous),
//                                        W = the convolution's weight [Cout = K][Cin = N] (N contiguous: no per-step transposed copy)
// epilogue, each part optional (a NULL pointer switches it off):
//   v += C[m, n]                         the block's parked skip gradient (torchvision Bottleneck's identity: beta = 1)
//   v  = mask[m, n] > 0 ? v : 0          mask = the convolution's own input = the layer in front's post-ReLU output
//   out_skip[m, n] = bf16(v)             the gradient of that layer's residual input (may overwrite C in place: same index, same thread)
//   out[m, n] = bf16(v * scale[n])       the gradient after that layer's frozen-BN affine
// Workgroup tile TM x TN (64 x 64 in the step: >= 300 workgroups at every site shape of 2 clips, no K split; 128 x 128 / 64 x 128 for
// measurement, ocpg_gemm_dgrad_bn_tile), 4 waves
// as 2 x 2, each wave TM/2 x TN/2 = 32x32 MFMA accumulators; K step 64, two register sets in flight (the loads of step s + 2 are issued
// while step s computes), double-buffered LDS, one barrier per step.  The weight tile is staged [k][n] as it lies and its MFMA fragments
// (8 consecutive k of one n) are read with gfx950's transposing ds_read_b64_tr_b16 (conv3x3_mfma's BTR path).  The accumulators leave
// through LDS so that every thread handles 8 consecutive columns of one row: 16-byte loads of C and the mask, 16-byte stores.  Every
// output element is one fp32 chain over k in ascending order, whatever the tile: deterministic, and the same bits for every tile.
//
// The same tile code also serves the encoder FFN of the transformer (MODE below, bf16): linear2's input gradient with the bias + ReLU +
// dropout backward and the bias gradient's partial column sums in its epilogue (ocpg_gemm_dgrad_mask), and linear1 with bias + ReLU +
// dropout in its epilogue (ocpg_gemm_bias_relu_dropout_fwd; the weight [N][K] as it lies, plain fragment reads).  The MODE_BN
// instantiations are the kernels they were before the modes existed.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"
#include "h16_elem.h"
#include "philox.h"

namespace {

typedef ocpg_h16::h16x8 bf16x8;
typedef short s4 __attribute__((ext_vector_type(4)));
typedef ocpg_h16::f32x16 f32x16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 64, NT = 256;
constexpr int ALD = BK + 8;            // A image [m][k]: 144-byte rows (16-B aligned, rows 4 banks apart)

constexpr int DECLINE_SHAPE = -2000, DECLINE_ALIGN = -2001, DECLINE_DTYPE = -2002;

// storage type of a kernel (h16_elem.h) with the packed widening / RNE narrowing of this epilogue: all that differs between the types
struct Bf16 : ocpg_h16::Bf16 {
  static __device__ __forceinline__ void unpack8(const uint4 u, float (&f)[8]) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[i] = (uint32_t)__bfloat16_as_ushort(__float2bfloat16(f[2 * i])) | ((uint32_t)__bfloat16_as_ushort(__float2bfloat16(f[2 * i + 1])) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};
struct Fp16 : ocpg_h16::Fp16 {
  static __device__ __forceinline__ void unpack8(const uint4 u, float (&f)[8]) {
    const __half2* h = reinterpret_cast<const __half2*>(&u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float2 t = __half22float2(h[i]);
      f[2 * i] = t.x;
      f[2 * i + 1] = t.y;
    }
  }
  static __device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[i] = (uint32_t)__half_as_ushort(__float2half_rn(f[2 * i])) | ((uint32_t)__half_as_ushort(__float2half_rn(f[2 * i + 1])) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};

template <typename T>
struct EpiT {
  const T* c;      // may alias out_skip (not __restrict__)
  const T* mask;
  const float* scale;
  T* out;
  T* out_skip;
};
using Epi = EpiT<__hip_bfloat16>;

// What the tile code computes.  BN: the 1x1 input gradient above (epilogue EpiT).  The two FFN modes (FfnT, encoder FFN of the transformer):
//   FFN_MASK  out = bf16(v * scale * [mask > 0]) with a SCALAR scale, plus the partial column sums of that value (before narrowing) over
//             the row tile: linear2's input gradient with the bias + ReLU + dropout backward of the hidden map in its epilogue;
//   FFN_FWD   B = linear1's weight [N][K] as it lies (k contiguous: plain fragment reads), out = bf16(max(v + bias[n], 0) * keep),
//             keep drawn as fused_ln.hip's brd_fwd draws it (counter = element index / 4, offset0 + *rng_base).  round_v: v is rounded
//             to bf16 before the bias is added, which is the arithmetic of the pair it replaces (a bf16 GEMM result, then brd_fwd):
//             the same h wherever the two GEMMs' fp32 sums round to the same bf16 value.
constexpr int MODE_BN = 0, MODE_FFN_MASK = 1, MODE_FFN_FWD = 2;
template <typename T>
struct FfnT {
  const T* mask;               // FFN_MASK: the saved hidden map h
  const T* bias;               // FFN_FWD
  T* out;
  float* colsum;               // FFN_MASK: [mtiles][N], every element stored once
  float scale;                 // 1 / (1 - p)
  uint32_t thr;                // FFN_FWD: p * 2^32 (0: nothing is drawn)
  uint64_t seed, offset0;
  const uint64_t* rng_base;
  int round_v;                 // FFN_FWD: round v to bf16 before the bias (the pair's arithmetic)
};

// C and mask of 8 consecutive columns, loaded ahead of the arithmetic (all of a thread's loads in flight at once: the epilogue is the
// memory-bound part of the short-K sites)
struct In8 { uint4 c, y; };
template <typename T>
__device__ __forceinline__ In8 load8(const EpiT<T>& e, long long off) {
  In8 r{make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
  if (e.c) r.c = *reinterpret_cast<const uint4*>(e.c + off);
  if (e.mask) r.y = *reinterpret_cast<const uint4*>(e.mask + off);
  return r;
}

// 8 consecutive columns col .. col + 7 of one row; off = row * N + col
template <typename E>
__device__ __forceinline__ void epilogue8(const EpiT<typename E::T>& e, long long off, int col, float (&v)[8], const In8& in) {
  if (e.c) {
    float c[8];
    E::unpack8(in.c, c);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += c[i];
  }
  if (e.mask) {
    float y[8];
    E::unpack8(in.y, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = y[i] > 0.f ? v[i] : 0.f;           // ocpg_bn_act_bwd's test on the saved output
  }
  if (e.out_skip) *reinterpret_cast<uint4*>(e.out_skip + off) = E::pack8(v);
  if (e.scale) {
    const float4 s0 = reinterpret_cast<const float4*>(e.scale + col)[0], s1 = reinterpret_cast<const float4*>(e.scale + col)[1];
    v[0] *= s0.x, v[1] *= s0.y, v[2] *= s0.z, v[3] *= s0.w, v[4] *= s1.x, v[5] *= s1.y, v[6] *= s1.z, v[7] *= s1.w;
  }
  *reinterpret_cast<uint4*>(e.out + off) = E::pack8(v);
}

// grid: mtiles * ntiles workgroups (1-D)
template <typename E, int TM, int TN, int MODE = MODE_BN>
__device__ __forceinline__ void gemm_dgrad_bn_body(const typename E::T* __restrict__ a, const typename E::T* __restrict__ w,
                                                   const EpiT<typename E::T>& e, long long M, int N, int K, int mtiles, int ntiles,
                                                   const FfnT<typename E::T>& f = FfnT<typename E::T>{}) {
  using T = typename E::T;
  constexpr bool BNK = MODE == MODE_FFN_FWD;                // B lies [N][K]: staged [n][k] like A, read without the transposing loads
  constexpr int BLD = TN + 8;          // B image [k][n]: rows 16-B aligned, 4 banks apart
  constexpr int SLD = TN + 4;          // fp32 accumulator image [m][n] for the epilogue
  constexpr int WM = TM / 2, WN = TN / 2, IM = WM / 32, JN = WN / 32;     // wave tile and its 32x32 accumulators
  constexpr int A_L = TM * BK / 8 / NT;                    // 16-B loads per thread and K step
  constexpr int BSEG = TN / 8, BROWS = NT / BSEG, B_L = BNK ? TN * BK / 8 / NT : BK / BROWS;
  constexpr int B_SHORTS = BNK ? TN * ALD : BK * BLD;
  constexpr int SMEM_SHORTS = 2 * (TM * ALD + B_SHORTS);
  static_assert(TM * SLD * 2 <= SMEM_SHORTS, "the fp32 tile fits the staging buffers");
  __shared__ __attribute__((aligned(16))) short smem[SMEM_SHORTS];
  short (*As)[TM * ALD] = reinterpret_cast<short (*)[TM * ALD]>(smem);
  short (*Bs)[B_SHORTS] = reinterpret_cast<short (*)[B_SHORTS]>(smem + 2 * TM * ALD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;                 // wave tile: rows wm * WM .., columns wn * WN ..
  // consecutive workgroups land on different XCDs (round robin over 8): give each XCD a contiguous run of tiles, so the column tiles of
  // one row panel (which read the same A rows) share an L2
  const unsigned total = gridDim.x;
  unsigned t = blockIdx.x;
  if ((total & 7u) == 0) t = (t & 7u) * (total >> 3) + (t >> 3);
  const long long m0 = (long long)(t / ntiles) * TM;
  const int n0 = (int)(t % ntiles) * TN;
  const int ksteps = K / BK;

  // staging identity.  A: row arow + 32 i, 16-B segment aseg of the 64-wide K step; rows past M read row M - 1 (never stored).
  // B: k row kr + BROWS i, columns n0 + 8 bseg ..
  const int arow = tid >> 3, aseg = tid & 7, kr = tid / BSEG, bseg = tid % BSEG;
  const T* ap[A_L];
#pragma unroll
  for (int i = 0; i < A_L; ++i) {
    const long long r = min(m0 + arow + 32 * i, M - 1);
    ap[i] = a + r * K + aseg * 8;
  }
  // ([N][K] weight: row n0 + arow + 32 i, segment aseg, as A; N % TN == 0, no row to clamp)
  const T* wp = BNK ? w + (long long)(n0 + arow) * K + aseg * 8 : w + (long long)kr * N + n0 + bseg * 8;
  const long long wstep = BNK ? 32ll * K : (long long)BROWS * N;     // B rows between a thread's consecutive loads

  // register sets are native vectors: with HIP's uint4 (a class) the two sets lived in scratch
  auto fetch = [&](u32x4 (&Ra)[A_L], u32x4 (&Rb)[B_L], int s) __attribute__((always_inline)) {   // K step s, clamped (valid memory)
    const int ks = min(s, ksteps - 1);
#pragma unroll
    for (int i = 0; i < A_L; ++i) Ra[i] = *reinterpret_cast<const u32x4*>(ap[i] + ks * BK);
    const T* wk = BNK ? wp + ks * BK : wp + (long long)ks * BK * N;
#pragma unroll
    for (int i = 0; i < B_L; ++i) Rb[i] = *reinterpret_cast<const u32x4*>(wk + i * wstep);
  };
  auto park = [&](int buf, const u32x4 (&Ra)[A_L], const u32x4 (&Rb)[B_L]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < A_L; ++i) *reinterpret_cast<u32x4*>(&As[buf][(arow + 32 * i) * ALD + aseg * 8]) = Ra[i];
#pragma unroll
    for (int i = 0; i < B_L; ++i) {
      if constexpr (BNK) *reinterpret_cast<u32x4*>(&Bs[buf][(arow + 32 * i) * ALD + aseg * 8]) = Rb[i];
      else *reinterpret_cast<u32x4*>(&Bs[buf][(kr + BROWS * i) * BLD + bseg * 8]) = Rb[i];
    }
  };

  f32x16 acc[IM * JN];
#pragma unroll
  for (int i = 0; i < IM * JN; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;                // fragment row (A) / column (B) and k-half of this lane
  // B fragment (8 consecutive k from k0 + 8 fh, column ncol0 + fr) out of the [k][n] image by two transposing reads: per 16-lane group a
  // 4-row x 16-column block, lane 4q + p addresses row q, columns 4p .. 4p + 3, lane i receives column i (EXEC is all ones here)
  auto btr = [&](int buf, int k0, int ncol0) __attribute__((always_inline)) -> bf16x8 {
    const int li = lane & 15, grp = lane >> 4;
    const short* p = &Bs[buf][(k0 + 8 * fh + (li >> 2)) * BLD + ncol0 + 16 * (grp & 1) + 4 * (li & 3)];
    const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
    const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(p + 4 * BLD));
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3]; r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
  };
  auto compute = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      bf16x8 af[IM], bf[JN];
#pragma unroll
      for (int i = 0; i < IM; ++i) af[i] = *reinterpret_cast<const bf16x8*>(&As[buf][(wm * WM + i * 32 + fr) * ALD + kk * 16 + fh * 8]);
#pragma unroll
      for (int j = 0; j < JN; ++j) {
        if constexpr (BNK) bf[j] = *reinterpret_cast<const bf16x8*>(&Bs[buf][(wn * WN + j * 32 + fr) * ALD + kk * 16 + fh * 8]);
        else bf[j] = btr(buf, kk * 16, wn * WN + j * 32);
      }
#pragma unroll
      for (int i = 0; i < IM; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j) acc[i * JN + j] = E::mfma(af[i], bf[j], acc[i * JN + j]);
    }
  };

  // two register sets: the loads of step s + 2 fly while step s computes and step s + 1 is parked (fetches are unconditional -- past the
  // end they re-read the last step and are parked into a buffer nobody reads -- so the wait before a park never covers the younger
  // loads).  ksteps is even (the host checks).
  u32x4 R0a[A_L], R0b[B_L], R1a[A_L], R1b[B_L];
  fetch(R0a, R0b, 0);
  fetch(R1a, R1b, 1);
  // FFN_MASK: the tile's share of the mask (thread = row group tid / BSEG, 8 columns, as its epilogue below) is requested right behind
  // the first two operand fetches (younger than both: no wait of the first K step covers it), so that this HBM read runs under the K loop
  constexpr int NQM = MODE == MODE_FFN_MASK ? TM * TN / 8 / NT : 1;
  u32x4 ymask[NQM];
  if constexpr (MODE == MODE_FFN_MASK) {
#pragma unroll
    for (int q = 0; q < NQM; ++q) {
      const long long grow = min(m0 + tid / BSEG + (NT / BSEG) * q, M - 1);        // rows past M re-read row M - 1 (never used)
      ymask[q] = *reinterpret_cast<const u32x4*>(f.mask + grow * N + n0 + (tid % BSEG) * 8);
    }
  }
  park(0, R0a, R0b);
  __syncthreads();
  for (int s = 0; s < ksteps; s += 2) {                    // R1 holds step s + 1, R0 (step s, parked) takes step s + 2; then they swap
    fetch(R0a, R0b, s + 2);
    compute(0);
    park(1, R1a, R1b);                                     // buffer 1 was last read in step s - 1 (barrier since)
    __syncthreads();
    fetch(R1a, R1b, s + 3);
    compute(1);
    park(0, R0a, R0b);
    __syncthreads();
  }

  // ---- accumulators -> fp32 tile image [m][n] (32x32 MFMA C/D layout: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5));
  // the loop ended with a barrier, the staging buffers are free
  float* st = reinterpret_cast<float*>(smem);
  float* st0 = st + (wm * WM + 4 * fh) * SLD + wn * WN + fr;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float* p = st0 + ((r & 3) + 8 * (r >> 2)) * SLD;
#pragma unroll
    for (int i = 0; i < IM; ++i)
#pragma unroll
      for (int j = 0; j < JN; ++j) p[i * 32 * SLD + j * 32] = acc[i * JN + j][r];
  }
  __syncthreads();
  // ---- thread = (row, 8 consecutive columns), NQ of them per thread; every C / mask load is issued before the first store.  Rows past M
  // load nothing (at a ragged edge C is written in place by other threads: no thread reads an element it does not own)
  constexpr int NQ = TM * TN / 8 / NT;
  if constexpr (MODE == MODE_FFN_MASK) {
    // NT % BSEG == 0: a thread keeps its 8 columns for all its NQ rows (row group rg, rows rg + RG q) and sums them in ascending q
    constexpr int RG = NT / BSEG;
    const int rg = tid / BSEG, c8 = (tid % BSEG) * 8;
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int row = rg + RG * q;
      const long long grow = m0 + row;
      if (grow >= M) continue;
      const float4 x0 = *reinterpret_cast<const float4*>(&st[row * SLD + c8]), x1 = *reinterpret_cast<const float4*>(&st[row * SLD + c8 + 4]);
      float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w}, yv[8];
      E::unpack8(*reinterpret_cast<const uint4*>(&ymask[q]), yv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        v[i] = yv[i] > 0.f ? v[i] * f.scale : 0.f;
        cs[i] += v[i];
      }
      *reinterpret_cast<uint4*>(f.out + grow * N + n0 + c8) = E::pack8(v);
    }
    // the RG partial sums of a column through the (now free) tile image, added in ascending row group by one thread: a fixed order
    static_assert(RG <= TM, "the partial sums fit the tile image");
    __syncthreads();
    *reinterpret_cast<float4*>(&st[rg * SLD + c8]) = make_float4(cs[0], cs[1], cs[2], cs[3]);
    *reinterpret_cast<float4*>(&st[rg * SLD + c8 + 4]) = make_float4(cs[4], cs[5], cs[6], cs[7]);
    __syncthreads();
    if (tid < TN) {
      float sum = 0.f;
#pragma unroll
      for (int g = 0; g < RG; ++g) sum += st[g * SLD + tid];
      f.colsum[(long long)(t / ntiles) * N + n0 + tid] = sum;
    }
    return;
  } else if constexpr (MODE == MODE_FFN_FWD) {
    const uint64_t offset = f.offset0 + (f.rng_base ? *f.rng_base : 0ull);
    const int c8 = (tid % BSEG) * 8;
    float bv[8];
    E::unpack8(*reinterpret_cast<const uint4*>(f.bias + n0 + c8), bv);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int row = tid / BSEG + (NT / BSEG) * q;
      const long long grow = m0 + row;
      if (grow >= M) continue;
      const float4 x0 = *reinterpret_cast<const float4*>(&st[row * SLD + c8]), x1 = *reinterpret_cast<const float4*>(&st[row * SLD + c8 + 4]);
      float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      if (f.round_v) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __bfloat162float(__float2bfloat16(v[i]));
      }
      const long long off = grow * N + n0 + c8;
      // fused_ln.hip's keep4 on counters off / 4 and off / 4 + 1, in scalars (its array form goes to scratch); p = 0 draws nothing
      uint4 r0 = make_uint4(~0u, ~0u, ~0u, ~0u), r1 = r0;
      if (f.thr != 0u) {
        const uint2 key = make_uint2((uint32_t)f.seed, (uint32_t)(f.seed >> 32));
        const uint64_t i4 = (uint64_t)off / 4;
        r0 = ocpg_dev::philox(key, make_uint4((uint32_t)i4, (uint32_t)(i4 >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)));
        r1 = ocpg_dev::philox(key, make_uint4((uint32_t)(i4 + 1), (uint32_t)((i4 + 1) >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)));
      }
      const uint32_t rr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i] + bv[i], 0.f) * (rr[i] >= f.thr ? f.scale : 0.f);
      *reinterpret_cast<uint4*>(f.out + off) = E::pack8(v);
    }
    return;
  }
  In8 in[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int idx = tid + q * NT;
    const long long grow = m0 + idx / BSEG;
    in[q] = grow < M ? load8(e, grow * N + n0 + (idx % BSEG) * 8) : In8{make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int idx = tid + q * NT, row = idx / BSEG, c8 = (idx % BSEG) * 8;
    const long long grow = m0 + row;
    if (grow >= M) continue;
    const float4 x0 = *reinterpret_cast<const float4*>(&st[row * SLD + c8]), x1 = *reinterpret_cast<const float4*>(&st[row * SLD + c8 + 4]);
    float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    epilogue8<E>(e, grow * N + n0 + c8, n0 + c8, v, in[q]);
  }
}

template <int TM, int TN>
__global__ __launch_bounds__(NT) void gemm_dgrad_bn(const __hip_bfloat16* __restrict__ a, const __hip_bfloat16* __restrict__ w, Epi e,
                                                    long long M, int N, int K, int mtiles, int ntiles) {
  gemm_dgrad_bn_body<Bf16, TM, TN>(a, w, e, M, N, K, mtiles, ntiles);
}

template <int TM, int TN>
__global__ __launch_bounds__(NT) void gemm_dgrad_bn_f16(const __half* __restrict__ a, const __half* __restrict__ w, EpiT<__half> e,
                                                        long long M, int N, int K, int mtiles, int ntiles) {
  gemm_dgrad_bn_body<Fp16, TM, TN>(a, w, e, M, N, K, mtiles, ntiles);
}

template <int TM, int TN, int MODE>
__global__ __launch_bounds__(NT) void gemm_ffn(const __hip_bfloat16* __restrict__ a, const __hip_bfloat16* __restrict__ w, FfnT<__hip_bfloat16> f,
                                               long long M, int N, int K, int mtiles, int ntiles) {
  gemm_dgrad_bn_body<Bf16, TM, TN, MODE>(a, w, Epi{}, M, N, K, mtiles, ntiles, f);
}

constexpr int TILE_M[3] = {128, 64, 64}, TILE_N[3] = {128, 128, 64};

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

// 64 x 64 wherever N % 64 == 0; -1: shape not served.  At every ResNet-101 site shape (tools/bench_dgrad_bn.py) 64 x 64 was the fastest
// tile on warm operands and within 10 % of the fastest on cold ones: layer3 / layer4 at 2 clips fill the chip without a K split (>= 300
// workgroups),
// and at 2-4 workgroups per CU the loads of one hide behind the MFMAs of another.  The larger tiles stay selectable for that sweep.
extern "C" int ocpg_gemm_dgrad_bn_tile(long long M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || N % TILE_N[2] != 0 || K % (2 * BK) != 0) return -1;
  return 2;
}

extern "C" int ocpg_gemm_dgrad_bn(const void* a, const void* w, const void* c, const void* mask, const float* scale, void* out, void* out_skip,
                                  long long M, int N, int K, int dtype, int tile, void* stream) {
  if (dtype != 1 && dtype != 2) return DECLINE_DTYPE;
  if (M < 0 || N <= 0 || K <= 0) return -1007;
  if (tile < 0 || tile > 2) return -1011;
  if (N % TILE_N[tile] != 0 || K % (2 * BK) != 0) return DECLINE_SHAPE;
  if (!a) return -1001;
  if (!w) return -1002;
  if (!out) return -1006;
  const void* ptrs[] = {a, w, c, mask, scale, out, out_skip};
  for (const void* p : ptrs)
    if (p && !aligned16(p)) return DECLINE_ALIGN;
  if (M == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const int mtiles = (int)((M + TILE_M[tile] - 1) / TILE_M[tile]), ntiles = N / TILE_N[tile];
  const dim3 grid((unsigned)(mtiles * ntiles)), block(NT);
  if (dtype == 2) {
    const EpiT<__half> e{(const __half*)c, (const __half*)mask, scale, (__half*)out, (__half*)out_skip};
    const __half *ap = (const __half*)a, *wp = (const __half*)w;
    if (tile == 0) gemm_dgrad_bn_f16<128, 128><<<grid, block, 0, st>>>(ap, wp, e, M, N, K, mtiles, ntiles);
    else if (tile == 1) gemm_dgrad_bn_f16<64, 128><<<grid, block, 0, st>>>(ap, wp, e, M, N, K, mtiles, ntiles);
    else gemm_dgrad_bn_f16<64, 64><<<grid, block, 0, st>>>(ap, wp, e, M, N, K, mtiles, ntiles);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : -(int)err;
  }
  const Epi e{(const __hip_bfloat16*)c, (const __hip_bfloat16*)mask, scale, (__hip_bfloat16*)out, (__hip_bfloat16*)out_skip};
  const __hip_bfloat16 *ap = (const __hip_bfloat16*)a, *wp = (const __hip_bfloat16*)w;
  if (tile == 0) gemm_dgrad_bn<128, 128><<<grid, block, 0, st>>>(ap, wp, e, M, N, K, mtiles, ntiles);
  else if (tile == 1) gemm_dgrad_bn<64, 128><<<grid, block, 0, st>>>(ap, wp, e, M, N, K, mtiles, ntiles);
  else gemm_dgrad_bn<64, 64><<<grid, block, 0, st>>>(ap, wp, e, M, N, K, mtiles, ntiles);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : -(int)err;
}

namespace {

template <int MODE>
int launch_ffn(const void* a, const void* w, const FfnT<__hip_bfloat16>& f, long long M, int N, int K, int tile, hipStream_t st) {
  const int mtiles = (int)((M + TILE_M[tile] - 1) / TILE_M[tile]), ntiles = N / TILE_N[tile];
  const dim3 grid((unsigned)(mtiles * ntiles)), block(NT);
  const __hip_bfloat16 *ap = (const __hip_bfloat16*)a, *wp = (const __hip_bfloat16*)w;
  if (tile == 0) gemm_ffn<128, 128, MODE><<<grid, block, 0, st>>>(ap, wp, f, M, N, K, mtiles, ntiles);
  else if (tile == 1) gemm_ffn<64, 128, MODE><<<grid, block, 0, st>>>(ap, wp, f, M, N, K, mtiles, ntiles);
  else gemm_ffn<64, 64, MODE><<<grid, block, 0, st>>>(ap, wp, f, M, N, K, mtiles, ntiles);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : -(int)err;
}

}  // namespace

extern "C" int ocpg_gemm_dgrad_mask(const void* a, const void* w, const void* mask, float scale, void* out, float* colsum_part, long long M, int N,
                                    int K, int dtype, int tile, void* stream) {
  if (dtype != 1) return DECLINE_DTYPE;
  if (M < 0 || N <= 0 || K <= 0) return -1007;
  if (tile < 0 || tile > 2) return -1011;
  if (N % TILE_N[tile] != 0 || K % (2 * BK) != 0) return DECLINE_SHAPE;
  if (!a) return -1001;
  if (!w) return -1002;
  if (!mask) return -1003;
  if (!out) return -1006;
  if (!colsum_part) return -1008;
  const void* ptrs[] = {a, w, mask, out, colsum_part};
  for (const void* p : ptrs)
    if (!aligned16(p)) return DECLINE_ALIGN;
  if (M == 0) return 0;
  const FfnT<__hip_bfloat16> f{(const __hip_bfloat16*)mask, nullptr, (__hip_bfloat16*)out, colsum_part, scale, 0u, 0ull, 0ull, nullptr, 0};
  return launch_ffn<MODE_FFN_MASK>(a, w, f, M, N, K, tile, (hipStream_t)stream);
}

extern "C" int ocpg_gemm_bias_relu_dropout_fwd(const void* x, const void* w, const void* bias, float p, unsigned long long seed,
                                               unsigned long long offset, const unsigned long long* rng_base, void* h, long long M, int N, int K,
                                               int dtype, int tile, int round_gemm, void* stream) {
  if (dtype != 1) return DECLINE_DTYPE;
  if (M < 0 || N <= 0 || K <= 0) return -1007;
  if (!(p >= 0.f && p < 1.f)) return -1009;
  if (tile < 0 || tile > 2) return -1011;
  if (N % TILE_N[tile] != 0 || K % (2 * BK) != 0) return DECLINE_SHAPE;
  if (!x) return -1001;
  if (!w) return -1002;
  if (!bias) return -1003;
  if (!h) return -1006;
  const void* ptrs[] = {x, w, bias, h};
  for (const void* q : ptrs)
    if (!aligned16(q)) return DECLINE_ALIGN;
  if (M == 0) return 0;
  uint32_t thr = 0u;                                       // fused_ln.hip's threshold(p)
  if (p > 0.f) {
    const double t = (double)p * 4294967296.0;
    thr = t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
  }
  const FfnT<__hip_bfloat16> f{nullptr, (const __hip_bfloat16*)bias, (__hip_bfloat16*)h, nullptr, 1.f / (1.f - p), thr, seed, offset,
                               (const uint64_t*)rng_base, round_gemm != 0};
  return launch_ffn<MODE_FFN_FWD>(x, w, f, M, N, K, tile, (hipStream_t)stream);
}
