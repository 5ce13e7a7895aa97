// The text gate of the vision-language fusion (models/segmentation.py: VisionLanguageFusionModule) as ONE kernel forward and a pair of
// kernels backward, for bf16 / fp16 autocast, C = 256, 8 heads of 32 and at most 16 text keys.
//
// The module computes, per visual token x (a 256-vector),  out = x * (Wo . attention(Wq x + bq; k, v) + bo).  With a handful of keys the
// two 256x256 projections are folded into the TEXT side: per clip b, key k, head h
//     K'[b, k*8+h, :] = Wq_h^T k[b,k,h,:]      c[b, k*8+h] = bq_h . k[b,k,h,:]      V'[b, k*8+h, :] = Wo[:, h-slice] v[b,k,h,:]
// (built by the caller with ordinary tensor ops; rows are KEY-major, n = k*8 + h), and then per token
//     s[n] = scale * (x . K'[n] + c[n]),   P = softmax over the keys of each head (padded keys masked),   a = sum_n P[n] V'[n] + bo,
//     out = x * a.
// Rounding points, as on the unfused path: x is rounded to the 16-bit type as the MFMA operand; scores, softmax and a are fp32 (P enters
// the second product as a hi + lo pair of 16-bit values, i.e. with ~16 mantissa bits); a is rounded ONCE to the 16-bit type and
// multiplied with the fp32 x.
//
// Layout.  Everything is computed TRANSPOSED, tokens on the MFMA column (lane & 15), with v_mfma_f32_16x16x32: a wave owns 16 tokens and
// lane (r = lane & 15, q = lane >> 4) holds x[token r][16 cb + 4 q .. + 3] for cb = 0..15 as sixteen float4 -- which is at once
//   * the B operand of  S^T[n, tok] = K'[n, :] . x[tok, :]  (the sum index may be permuted at will as long as both operands agree: the
//     k-step of 32 channels takes the lane's two float4 of channel blocks 2s and 2s+1),
//   * the C/D layout (row = 4 q + i, column = r) of  a^T[ch, tok] = V'^T[ch, :] . P^T[:, tok], so the epilogue multiplies register by
//     register and stores float4.
// S^T comes out with n = 16 nb + 4 q + i in register i of block nb: key = 2 nb + (q >> 1), head = 4 (q & 1) + i.  The softmax over the keys
// of a head is a reduction over nb (registers of one lane) and ONE exchange with lane ^ 32; and that C/D layout is again the B operand of the
// next product (k-step s = blocks 2s, 2s+1) with no lane movement.  K' and V' live in LDS for the workgroup's lifetime as plain
// [n][256] rows of 544 bytes (512 + 32: the transposing reads are conflict-free, the row reads 2-way); products that sum over channels
// read rows (ds_read_b64), products that sum over n read the same image with ds_read_b64_tr_b16 (EXEC is all ones: the tile loop is
// wave-uniform, ragged tiles clamp their addresses and only predicate the stores).
//
// Backward.  k_dx recomputes P and a, forms da = round16(g * x), dP^T = V' . da^T (row reads), dZ = scale * P * (dP - sum_keys P dP),
// dx = g * a16 + K'^T . dZ^T (transposing reads, accumulated onto the direct term) and leaves P and dZ as 16-bit [token][n] rows in a
// workspace.  k_params then forms the sums over tokens, dV' = P^T . da, dK' = dZ^T . x16, dc = sum dZ, dbo = sum da, as per-workgroup fp32
// PARTIALS over token ranges (no atomics: deterministic); the caller adds the partials with one sum(0).  The token sums are a second kernel
// because their fp32 accumulators (2 x 128 x 256 per workgroup = 256 KB) do not fit a CU next to the 136-KB operand images.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"
#include "h16_elem.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int C = 256;          // channels
constexpr int H = 8;            // heads (a row of K' / V' is n = key * 8 + head)
constexpr int RS = 544;         // bytes per LDS row of K' / V'
constexpr int NT = 512;         // threads of the forward kernel: 8 waves of 16 tokens
constexpr int DNT = 256;        // threads of the dx kernel: 4 waves, one per SIMD (its live set needs more than 256 registers)
constexpr int PNT = 256;        // threads of the parameter kernel
constexpr int PCH = 128;        // channels per workgroup of the parameter kernel
constexpr int PRS = 80;         // bytes per LDS row of its [column][32 tokens] tiles (64 + 16)
constexpr int MAX_SPLITS = 32;

struct Bf : ocpg_h16::Bf16 {
  static __device__ __forceinline__ f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
};

struct Hf : ocpg_h16::Fp16 {
  static __device__ __forceinline__ f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(unsigned short b) { return __half2float(__ushort_as_half(b)); }
};

template <typename E> __device__ __forceinline__ s16x4 pack4(f32x4 v) {
  s16x4 o;
  o[0] = (short)E::bits(v[0]);
  o[1] = (short)E::bits(v[1]);
  o[2] = (short)E::bits(v[2]);
  o[3] = (short)E::bits(v[3]);
  return o;
}

template <typename E> __device__ __forceinline__ f32x4 widen4(s16x4 v) {
  f32x4 o;
  o[0] = E::widen((unsigned short)v[0]);
  o[1] = E::widen((unsigned short)v[1]);
  o[2] = E::widen((unsigned short)v[2]);
  o[3] = E::widen((unsigned short)v[3]);
  return o;
}

__device__ __forceinline__ s16x8 cat(s16x4 a, s16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

__device__ __forceinline__ s16x4 tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// LDS of the token kernels: K' image, V' image, cs[NP] = scale * c or -inf (padded / masked key), bo[256]
template <int NB> struct Smem {
  static constexpr int NP = 16 * NB;
  static constexpr int IMG = NP * RS;
  static constexpr int CS = 2 * IMG;
  static constexpr int BO = CS + NP * 4;
  static constexpr int BYTES = BO + C * 4;
};

template <int NB, int THREADS>
__device__ __forceinline__ void stage(unsigned char* sm, const short* Kp, const short* Vp, const float* cvec, const float* bo,
                                      const unsigned char* pad, float scale, int Lk, int b) {
  using S = Smem<NB>;
  const int N = H * Lk;
  const uint4* kg = reinterpret_cast<const uint4*>(Kp + (size_t)b * N * C);
  const uint4* vg = reinterpret_cast<const uint4*>(Vp + (size_t)b * N * C);
  for (int u = threadIdx.x; u < S::NP * 32; u += THREADS) {
    const int row = u >> 5, ch = u & 31;
    uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
    if (row < N) {
      kv = kg[row * 32 + ch];
      vv = vg[row * 32 + ch];
    }
    *reinterpret_cast<uint4*>(sm + row * RS + ch * 16) = kv;
    *reinterpret_cast<uint4*>(sm + S::IMG + row * RS + ch * 16) = vv;
  }
  float* cs = reinterpret_cast<float*>(sm + S::CS);
  for (int n = threadIdx.x; n < S::NP; n += THREADS) {
    const int key = n >> 3;
    const bool dead = key >= Lk || (pad != nullptr && pad[b * Lk + key] != 0);
    cs[n] = dead ? -INFINITY : scale * cvec[(size_t)b * N + n];
  }
  float* bos = reinterpret_cast<float*>(sm + S::BO);
  for (int i = threadIdx.x; i < C; i += THREADS) bos[i] = bo[i];
  __syncthreads();
}

// out[nb] (+)= img[16 nb + 4 q + i, :] . f[:, token r]: the products that sum over the 256 channels; f = the lane's 16-bit x-layout values
template <typename E, int NB>
__device__ __forceinline__ void row_product(const unsigned char* img, const s16x4 (&f)[16], int r, int q, f32x4 (&out)[NB]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) out[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const s16x8 bf = cat(f[2 * s], f[2 * s + 1]);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const unsigned char* p = img + (16 * nb + r) * RS + (32 * s + 4 * q) * 2;
      const s16x8 af = cat(*reinterpret_cast<const s16x4*>(p), *reinterpret_cast<const s16x4*>(p + 32));
      out[nb] = E::mfma(af, bf, out[nb]);
    }
    __builtin_amdgcn_sched_barrier(0);          // keep the operand reads of later k-steps from being hoisted (register pressure)
  }
}

// acc[cb] += img^T[16 cb + 4 q + i, :] . v[:, token r]: the products that sum over n; v = the lane's C/D-layout values of a row product.
// HILO: v enters as hi + lo (two MFMAs per operand read).
template <typename E, int NB, bool HILO>
__device__ __forceinline__ void col_product(const unsigned char* img, const f32x4 (&v)[NB], int r, int q, f32x4 (&acc)[16]) {
#pragma unroll
  for (int s = 0; s < NB / 2; ++s) {
    const s16x4 h0 = pack4<E>(v[2 * s]), h1 = pack4<E>(v[2 * s + 1]);
    const s16x8 hi = cat(h0, h1);
    s16x8 lo = hi;
    if (HILO) lo = cat(pack4<E>(v[2 * s] - widen4<E>(h0)), pack4<E>(v[2 * s + 1] - widen4<E>(h1)));
    const unsigned char* base = img + (32 * s + 4 * q + (r >> 2)) * RS + (4 * (r & 3)) * 2;
#pragma unroll
    for (int cb = 0; cb < 16; ++cb) {
      const s16x8 af = cat(tr_read(base + cb * 32), tr_read(base + 16 * RS + cb * 32));
      acc[cb] = E::mfma(af, hi, acc[cb]);
      if (HILO) acc[cb] = E::mfma(af, lo, acc[cb]);
      if ((cb & 3) == 3) __builtin_amdgcn_sched_barrier(0);          // at most four blocks' operand reads in flight (register pressure)
    }
  }
}

// P[nb][i] = softmax over the keys of head 4 (q & 1) + i of scale * (S + c), S in P on entry
template <int NB> __device__ __forceinline__ void softmax(const unsigned char* sm, float scale, int q, f32x4 (&P)[NB]) {
  const float* cs = reinterpret_cast<const float*>(sm + Smem<NB>::CS);
  f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const f32x4 c4 = *reinterpret_cast<const f32x4*>(cs + 16 * nb + 4 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      P[nb][i] = fmaf(P[nb][i], scale, c4[i]);
      m[i] = fmaxf(m[i], P[nb][i]);
    }
  }
  f32x4 den = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = fmaxf(m[i], __shfl_xor(m[i], 32));
    if (m[i] == -INFINITY) m[i] = 0.f;          // every key of the clip masked: P = 0
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      P[nb][i] = __expf(P[nb][i] - m[i]);
      den[i] += P[nb][i];
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    den[i] += __shfl_xor(den[i], 32);
    den[i] = den[i] > 0.f ? 1.f / den[i] : 0.f;
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) P[nb][i] *= den[i];
}

template <typename E, int NB>
__global__ __launch_bounds__(NT) void k_fwd(const float* __restrict__ x, const short* __restrict__ Kp, const short* __restrict__ Vp,
                                            const float* __restrict__ cvec, const float* __restrict__ bo,
                                            const unsigned char* __restrict__ pad, float scale, int L, int Lk, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  using S = Smem<NB>;
  const int b = blockIdx.y;
  stage<NB, NT>(sm, Kp, Vp, cvec, bo, pad, scale, Lk, b);
  const float* bos = reinterpret_cast<const float*>(sm + S::BO);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int tiles = (L + 15) >> 4;
  const int t0 = (int)((long long)blockIdx.x * tiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * tiles / gridDim.x);
  for (int tile = t0 + wave; tile < t1; tile += NT / 64) {            // wave-uniform
    const int tok = tile * 16 + r, tc = tok < L ? tok : L - 1;
    const size_t off = ((size_t)b * L + tc) * C + 4 * q;
    f32x4 xv[16];
#pragma unroll
    for (int cb = 0; cb < 16; ++cb) xv[cb] = *reinterpret_cast<const f32x4*>(x + off + 16 * cb);
    f32x4 P[NB];
    {
      s16x4 xf[16];
#pragma unroll
      for (int cb = 0; cb < 16; ++cb) xf[cb] = pack4<E>(xv[cb]);
      row_product<E, NB>(sm, xf, r, q, P);
    }
    softmax<NB>(sm, scale, q, P);
    f32x4 acc[16];
#pragma unroll
    for (int cb = 0; cb < 16; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    col_product<E, NB, true>(sm + S::IMG, P, r, q, acc);
    if (tok < L) {
#pragma unroll
      for (int cb = 0; cb < 16; ++cb) {
        const f32x4 a16 = widen4<E>(pack4<E>(acc[cb] + *reinterpret_cast<const f32x4*>(bos + 16 * cb + 4 * q)));
        *reinterpret_cast<f32x4*>(out + off + 16 * cb) = xv[cb] * a16;
      }
    }
  }
}

template <typename E, int NB>
__global__ __launch_bounds__(DNT) void k_dx(const float* __restrict__ x, const float* __restrict__ g, const short* __restrict__ Kp,
                                           const short* __restrict__ Vp, const float* __restrict__ cvec, const float* __restrict__ bo,
                                           const unsigned char* __restrict__ pad, float scale, int L, int Lk, float* __restrict__ dx,
                                           short* __restrict__ P16, short* __restrict__ Z16) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  using S = Smem<NB>;
  const int b = blockIdx.y;
  stage<NB, DNT>(sm, Kp, Vp, cvec, bo, pad, scale, Lk, b);
  const float* bos = reinterpret_cast<const float*>(sm + S::BO);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const int tiles = (L + 15) >> 4;
  const int t0 = (int)((long long)blockIdx.x * tiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * tiles / gridDim.x);
  for (int tile = t0 + wave; tile < t1; tile += DNT / 64) {            // wave-uniform
    const int tok = tile * 16 + r, tc = tok < L ? tok : L - 1;
    const size_t off = ((size_t)b * L + tc) * C + 4 * q;
    f32x4 P[NB];
    f32x4 acc[16];          // a, then g * a16 (the direct term of dx), then dx
    s16x4 daf[16];          // da = round16(g * x)
    {
      f32x4 xv[16];
#pragma unroll
      for (int cb = 0; cb < 16; ++cb) xv[cb] = *reinterpret_cast<const f32x4*>(x + off + 16 * cb);
      {
        s16x4 xf[16];
#pragma unroll
        for (int cb = 0; cb < 16; ++cb) xf[cb] = pack4<E>(xv[cb]);
        row_product<E, NB>(sm, xf, r, q, P);
      }
      softmax<NB>(sm, scale, q, P);
#pragma unroll
      for (int cb = 0; cb < 16; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      col_product<E, NB, true>(sm + S::IMG, P, r, q, acc);
#pragma unroll
      for (int cb = 0; cb < 16; ++cb) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + off + 16 * cb);
        const f32x4 a16 = widen4<E>(pack4<E>(acc[cb] + *reinterpret_cast<const f32x4*>(bos + 16 * cb + 4 * q)));
        acc[cb] = gv * a16;
        daf[cb] = pack4<E>(gv * xv[cb]);
      }
    }
    f32x4 dZ[NB];
    row_product<E, NB>(sm + S::IMG, daf, r, q, dZ);         // dP
    f32x4 D = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) D += P[nb] * dZ[nb];
#pragma unroll
    for (int i = 0; i < 4; ++i) D[i] += __shfl_xor(D[i], 32);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) dZ[nb] = scale * P[nb] * (dZ[nb] - D);
    if (tok < L) {
      const size_t wo = ((size_t)b * L + tok) * S::NP + 4 * q;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        *reinterpret_cast<s16x4*>(P16 + wo + 16 * nb) = pack4<E>(P[nb]);
        *reinterpret_cast<s16x4*>(Z16 + wo + 16 * nb) = pack4<E>(dZ[nb]);
      }
    }
    col_product<E, NB, false>(sm, dZ, r, q, acc);
    if (tok < L) {
#pragma unroll
      for (int cb = 0; cb < 16; ++cb) *reinterpret_cast<f32x4*>(dx + off + 16 * cb) = acc[cb];
    }
  }
}

// Sums over tokens.  grid (splits, 4, B): blockIdx.y = 2 * role + channel half; role 0: dK' = dZ16^T . round16(x) and dc = sum dZ16,
// role 1: dV' = P16^T . round16(g * x) and dbo = sum round16(g * x).  A workgroup walks its token range in chunks of 32 (the MFMA's sum
// index): both operands of a chunk are parked in LDS as [column][32 tokens] rows, the next chunk's global loads are in flight meanwhile.
// part [splits][B][W], W = 2 NP 256 + NP + 256: dK' [NP][256], dV' [NP][256], dc [NP], dbo [256]; every element is written by exactly
// one workgroup (zeros from a workgroup without tokens).
template <typename E, int NB>
__global__ __launch_bounds__(PNT) void k_params(const float* __restrict__ x, const float* __restrict__ g, const short* __restrict__ P16,
                                                const short* __restrict__ Z16, int L, float* __restrict__ part) {
  constexpr int NP = 16 * NB, UPT = NP / 4, NU = NB / 2;
  __shared__ __attribute__((aligned(16))) unsigned char At[NP * PRS];
  __shared__ __attribute__((aligned(16))) unsigned char Bt[PCH * PRS];
  const int tid = threadIdx.x, role = blockIdx.y >> 1, half = blockIdx.y & 1, b = blockIdx.z, B = gridDim.z;
  const int wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int chunks = (L + 31) >> 5;
  const int c0 = (int)((long long)blockIdx.x * chunks / gridDim.x), c1 = (int)((long long)(blockIdx.x + 1) * chunks / gridDim.x);
  const short* A16 = (role ? P16 : Z16) + (size_t)b * L * NP;
  const float* xb = x + (size_t)b * L * C + half * PCH;
  const float* gb = g + (size_t)b * L * C + half * PCH;
  const int stok = tid >> 3, scol = (tid & 7) * 16;         // staging: 8 threads x 16 channels per token

  f32x4 acc[NB][2];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb][0] = acc[nb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float colsum = 0.f;
  f32x4 bv[4];
  s16x4 av[NU];

  auto load = [&](int chunk) {
    const int tok = chunk * 32 + stok;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (tok < L) {
        bv[j] = *reinterpret_cast<const f32x4*>(xb + (size_t)tok * C + scol + 4 * j);
        if (role) bv[j] *= *reinterpret_cast<const f32x4*>(gb + (size_t)tok * C + scol + 4 * j);
      }
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + PNT * i, t = chunk * 32 + u / UPT, n4 = u % UPT;
      av[i] = s16x4{0, 0, 0, 0};
      if (t < L) av[i] = *reinterpret_cast<const s16x4*>(A16 + (size_t)t * NP + 4 * n4);
    }
  };

  if (c0 < c1) load(c0);
  for (int chunk = c0; chunk < c1; ++chunk) {
    __syncthreads();            // the previous chunk's reads of At / Bt are done
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const s16x4 h = pack4<E>(bv[j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) *reinterpret_cast<short*>(Bt + (scol + 4 * j + e) * PRS + stok * 2) = h[e];
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + PNT * i, t = u / UPT, n4 = u % UPT;
#pragma unroll
      for (int e = 0; e < 4; ++e) *reinterpret_cast<short*>(At + (4 * n4 + e) * PRS + t * 2) = av[i][e];
    }
    __syncthreads();
    if (chunk + 1 < c1) load(chunk + 1);
    if (tid < (role ? PCH : NP)) {          // dbo / dc: the column's 32 tokens
      const unsigned char* row = (role ? Bt : At) + tid * PRS;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const s16x8 v = *reinterpret_cast<const s16x8*>(row + 16 * j);
#pragma unroll
        for (int e = 0; e < 8; ++e) colsum += E::widen((unsigned short)v[e]);
      }
    }
#pragma unroll
    for (int cw = 0; cw < 2; ++cw) {
      const s16x8 bf = *reinterpret_cast<const s16x8*>(Bt + (16 * (2 * wave + cw) + r) * PRS + 16 * q);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const s16x8 af = *reinterpret_cast<const s16x8*>(At + (16 * nb + r) * PRS + 16 * q);
        acc[nb][cw] = E::mfma(af, bf, acc[nb][cw]);
      }
    }
  }

  constexpr int W = 2 * NP * C + NP + C;
  float* o = part + ((size_t)blockIdx.x * B + b) * W;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int cw = 0; cw < 2; ++cw)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[(size_t)role * NP * C + (16 * nb + 4 * q + i) * C + half * PCH + 16 * (2 * wave + cw) + r] = acc[nb][cw][i];
  if (role) {
    if (tid < PCH) o[2 * NP * C + NP + half * PCH + tid] = colsum;
  } else if (half == 0 && tid < NP) {
    o[2 * NP * C + tid] = colsum;
  }
}

inline int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

inline int blocks_of(int Lk) { return Lk <= 4 ? 2 : Lk <= 8 ? 4 : Lk <= 12 ? 6 : 8; }

inline bool served(int C_, int H_, int Lk, int B) { return C_ == C && H_ == H && Lk >= 1 && Lk <= 16 && B <= 65535; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int token_grid(int B, int L, int waves) {
  const int per = ((L + 15) / 16 + waves - 1) / waves;                // workgroup tiles of 16 tokens per wave
  const int cap = B >= 256 ? 1 : 256 / B;                             // about one workgroup per CU: each stages K' and V' once
  return per < cap ? per : cap;
}

// Kernels above the default 64-KB dynamic-LDS window opt in ONCE per instantiation and device (`done` is the caller's static table);
// a refusal is reported, not left to the launch.
inline int allow_lds(const void* kernel, size_t bytes, bool (&done)[64]) {
  if (bytes <= 64 * 1024) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
  if (dev >= 0 && done[dev]) return 0;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return -(int)e;
  if (dev >= 0) done[dev] = true;
  return 0;
}

template <typename E, int NB>
int launch_fwd(const float* x, const void* Kp, const void* Vp, const float* c, const float* bo, const unsigned char* pad, float scale, int B,
               int L, int Lk, float* out, hipStream_t st) {
  static bool done[64] = {};
  if (const int rc = allow_lds(reinterpret_cast<const void*>(k_fwd<E, NB>), Smem<NB>::BYTES, done)) return rc;
  k_fwd<E, NB><<<dim3(token_grid(B, L, NT / 64), B), NT, Smem<NB>::BYTES, st>>>(x, (const short*)Kp, (const short*)Vp, c, bo, pad, scale, L, Lk, out);
  return status();
}

template <typename E, int NB>
int launch_bwd(const float* x, const float* g, const void* Kp, const void* Vp, const float* c, const float* bo, const unsigned char* pad,
               float scale, int B, int L, int Lk, float* dx, float* part, void* ws, hipStream_t st) {
  short* P16 = (short*)ws;
  short* Z16 = P16 + (size_t)B * L * 16 * NB;
  static bool done[64] = {};
  if (const int rc = allow_lds(reinterpret_cast<const void*>(k_dx<E, NB>), Smem<NB>::BYTES, done)) return rc;
  k_dx<E, NB><<<dim3(token_grid(B, L, DNT / 64), B), DNT, Smem<NB>::BYTES, st>>>(x, g, (const short*)Kp, (const short*)Vp, c, bo, pad, scale, L, Lk, dx,
                                                                      P16, Z16);
  int rc = status();
  if (rc != 0) return rc;
  k_params<E, NB><<<dim3(ocpg_text_gate_splits(L), 4, B), PNT, 0, st>>>(x, g, P16, Z16, L, part);
  return status();
}

}  // namespace

#define TG_DISPATCH(FN, ...)                                                          \
  switch ((dtype == 2 ? 10 : 0) + blocks_of(Lk)) {                                    \
    case 2: return FN<Bf, 2>(__VA_ARGS__);                                            \
    case 4: return FN<Bf, 4>(__VA_ARGS__);                                            \
    case 6: return FN<Bf, 6>(__VA_ARGS__);                                            \
    case 8: return FN<Bf, 8>(__VA_ARGS__);                                            \
    case 12: return FN<Hf, 2>(__VA_ARGS__);                                           \
    case 14: return FN<Hf, 4>(__VA_ARGS__);                                           \
    case 16: return FN<Hf, 6>(__VA_ARGS__);                                           \
    default: return FN<Hf, 8>(__VA_ARGS__);                                           \
  }

extern "C" {

int ocpg_text_gate_rows(int Lk) { return Lk >= 1 && Lk <= 16 ? 16 * blocks_of(Lk) : 0; }

int ocpg_text_gate_splits(int L) {
  const int s = (L + 255) / 256;
  return s < 1 ? 1 : s > MAX_SPLITS ? MAX_SPLITS : s;
}

int ocpg_text_gate_fwd_h16(const float* x, const void* Kp, const void* Vp, const float* c, const float* bo, const unsigned char* key_pad,
                           float scale, int B, int L, int C_, int H_, int Lk, float* out, int dtype, void* stream) {
  if (dtype != 1 && dtype != 2) return -1014;
  if (B < 0 || L < 0) return -1008;
  if (!served(C_, H_, Lk, B) || !aligned16(x) || !aligned16(Kp) || !aligned16(Vp) || !aligned16(c) || !aligned16(bo) || !aligned16(out))
    return -2000;
  if (B == 0 || L == 0) return 0;
  if (!x) return -1001;
  if (!Kp) return -1002;
  if (!Vp) return -1003;
  if (!c) return -1004;
  if (!bo) return -1005;
  if (!out) return -1013;
  TG_DISPATCH(launch_fwd, x, Kp, Vp, c, bo, key_pad, scale, B, L, Lk, out, (hipStream_t)stream)
}

int ocpg_text_gate_bwd_h16(const float* x, const float* g, const void* Kp, const void* Vp, const float* c, const float* bo,
                           const unsigned char* key_pad, float scale, int B, int L, int C_, int H_, int Lk, float* dx, float* part, void* ws,
                           int dtype, void* stream) {
  if (dtype != 1 && dtype != 2) return -1017;
  if (B < 0 || L < 0) return -1009;
  if (!served(C_, H_, Lk, B) || !aligned16(x) || !aligned16(g) || !aligned16(Kp) || !aligned16(Vp) || !aligned16(c) || !aligned16(bo) ||
      !aligned16(dx) || !aligned16(part) || !aligned16(ws))
    return -2000;
  if (B == 0 || L == 0) return 0;
  if (!x) return -1001;
  if (!g) return -1002;
  if (!Kp) return -1003;
  if (!Vp) return -1004;
  if (!c) return -1005;
  if (!bo) return -1006;
  if (!dx) return -1014;
  if (!part) return -1015;
  if (!ws) return -1016;
  TG_DISPATCH(launch_bwd, x, g, Kp, Vp, c, bo, key_pad, scale, B, L, Lk, dx, part, ws, (hipStream_t)stream)
}

}  // extern "C"
