// Multi-head attention against 33..128 keys (head_dim 32, H <= 8), forward and backward: the long-caption form of
// csrc/attn_smallk.hip.  The reference tokenises with padding='longest' and no truncation (models/text_encoder/tokenizer.py:146), so
// one caption of ~30 words in a batch gives every fusion call of the step (models/segmentation.py:95-113) more than 32 text keys; a
// model built with more than 32 queries has the same key count in the decoder's self-attention (models/deformable_transformer.py:323-326).
// Same contract as the short-key kernels: [L, B, H*32] rows with any row stride, key padding, attention-weight dropout, fp32 / bf16 /
// fp16 storage with fp32 arithmetic.
//
// The short-key kernels hold all K and V of a batch element in LDS (2 * Lk * H * 36 floats) next to the backward's (p~, ds) park:
// 138 KiB of the CU's 160 KiB at Lk = 32, H = 8, so that layout cannot grow.  Here the keys are walked in CHUNKS of 32: a chunk of K
// and V is staged (fp32, head slices padded to 36 floats), used by every thread, and replaced by the next; K and V are Lk * B * C
// elements and stay in L2.
//
// Forward.  A workgroup = 256 / H query tokens x H heads of one batch element, a thread = one (token, head) with q and the output
// accumulator in registers; the online-softmax state (m, l, acc[32]) carries over the chunks.  Threads without a token still stage
// and meet every barrier (predicated, no early return).
//
// Backward.  D = sum_j p~_j dp~_j = sum_d dout_d out_d for a (token, head), with or without dropout (out = sum_j p~_j v_j), so the
// forward's output is an input here and ONE sweep over the chunks of a window suffices.  Token groups outer, chunks inner: per chunk a
// thread recomputes p from the saved log-sum-exp, forms ds, adds ds k_j into its dq registers (kept across the chunks) and parks (p~, ds)
// of the chunk in LDS; the threads then regroup as (head, channel) and add the group's tokens into register sums of dK / dV for the
// keys of the launch's window (at most 2 chunks = 64 keys), which live across `groups_per_block` token groups and are flushed with
// fp32 atomics: NT / C = 8 / H threads share a channel and split a group's tokens, each flushes its own sums, so a workgroup issues
// 8 / H atomics per (key, channel) -- one at H = 8.  Restaging K / V per token group costs 8 H global loads per thread and chunk
// against ~5000 FMAs of work on that chunk.  Keys past 64 are a SECOND launch over the window at key 64: it reads q, dout, out and
// lse again, recomputes D, and adds its dq share to what the first launch wrote (dq is written, then re-read: a 16-bit dq is
// rounded twice), which is why 128 keys cost twice what 64 do.
//
// Keys are handled four at a time: one Philox call yields the four keep decisions, and (p~, ds) are parked with 16-byte LDS stores
// (row stride 36 floats: conflict-free for those, and the (head, channel) threads read them back as broadcast float4).  Rows past Lk
// in the last block of four are zero in LDS and carry a -inf bias, so they contribute exactly nothing.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"
#include "philox.h"

namespace {

constexpr int HD = 32;        // head dimension
constexpr int HS = 36;        // LDS stride of a head slice / of a thread's parked chunk (floats)
constexpr int NT = 256;
constexpr int CH = 32;        // keys per chunk
constexpr int MAXK = 128;     // most keys served

template <typename T> struct Cvt;
template <> struct Cvt<float> {
  static __device__ __forceinline__ float to(float v) { return v; }
  static __device__ __forceinline__ float from(float v) { return v; }
};
template <> struct Cvt<__hip_bfloat16> {
  static __device__ __forceinline__ float to(__hip_bfloat16 v) { return __bfloat162float(v); }
  static __device__ __forceinline__ __hip_bfloat16 from(float v) { return __float2bfloat16(v); }
};
template <> struct Cvt<__half> {
  static __device__ __forceinline__ float to(__half v) { return __half2float(v); }
  static __device__ __forceinline__ __half from(float v) { return __float2half(v); }
};

template <typename T>
__device__ __forceinline__ void load_row(const T* p, float (&f)[HD]) {
#pragma unroll
  for (int d = 0; d < HD; ++d) f[d] = Cvt<T>::to(p[d]);
}

// keep-scales of the attention weights (rowh, j .. j + 3), j % 4 == 0: 1/(1-p) or 0 each; thr = p * 2^32 (0 = no dropout).
// Stream index rowh * 128 + j (injective for j < 128; csrc/philox.h), four consecutive indices per Philox call.
__device__ __forceinline__ float4 keep_scale4(uint64_t seed, uint64_t offset, uint64_t rowh, int j, uint32_t thr, float inv_keep) {
  if (thr == 0u) return make_float4(1.f, 1.f, 1.f, 1.f);
  const uint64_t idx = rowh * (uint64_t)MAXK + (uint64_t)j;
  const uint4 r = ocpg_dev::philox(make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)),
                                   make_uint4((uint32_t)(idx >> 2), (uint32_t)(idx >> 34), (uint32_t)offset, (uint32_t)(offset >> 32)));
  return make_float4(r.x >= thr ? inv_keep : 0.f, r.y >= thr ? inv_keep : 0.f, r.z >= thr ? inv_keep : 0.f, r.w >= thr ? inv_keep : 0.f);
}

// bias[j] = 0 or -inf (key padding) for j < Lk, -inf for Lk <= j < MAXK
__device__ __forceinline__ void stage_bias(const unsigned char* __restrict__ pad, int b, int Lk, float* bias) {
  if (threadIdx.x < MAXK) {
    const int j = threadIdx.x;
    bias[j] = (j >= Lk || (pad && pad[(long long)b * Lk + j])) ? -INFINITY : 0.f;
  }
}

// stage keys j0 .. j0 + n - 1 of batch element b into LDS (fp32, head slices padded); rows n .. n4 - 1 (n4 = n rounded up to 4) are zeroed.
// C divides NT (H is 1, 2, 4 or 8): a thread keeps its channel and walks the rows.
template <typename T>
__device__ __forceinline__ void stage_chunk(const T* __restrict__ k, long long ldk, const T* __restrict__ v, long long ldv, int b, int B, int H,
                                            int j0, int n, int n4, float* ks, float* vs) {
  const int C = H * HD;
  const int c = threadIdx.x % C, h = c / HD, d = c % HD;
  for (int j = threadIdx.x / C; j < n4; j += NT / C) {
    const int at = (j * H + h) * HS + d;
    const bool live = j < n;
    ks[at] = live ? Cvt<T>::to(k[((long long)(j0 + j) * B + b) * ldk + c]) : 0.f;
    vs[at] = live ? Cvt<T>::to(v[((long long)(j0 + j) * B + b) * ldv + c]) : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void attn_longk_fwd(const T* __restrict__ q, long long ldq, const T* __restrict__ k, long long ldk,
                                                     const T* __restrict__ v, long long ldv, const unsigned char* __restrict__ pad,
                                                     float scale, int Lq, int B, int H, int Lk, float pdrop, uint64_t seed,
                                                     uint64_t offset0, const uint64_t* __restrict__ rng_base, T* __restrict__ out,
                                                     long long ldo, float* __restrict__ lse) {
  const uint64_t offset = offset0 + (rng_base ? *rng_base : 0ull);      // graph replays: the step's base lives in device memory
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ks = smem;
  float* vs = ks + CH * H * HS;
  float* bias = vs + CH * H * HS;
  const int b = blockIdx.y;
  const int tok_per = NT / H;
  const int tl = threadIdx.x / H, h = threadIdx.x % H;
  const int tok = blockIdx.x * tok_per + tl;
  const bool active = tok < Lq;                                         // no early return: every thread stages and meets the barriers
  const long long row = (long long)(active ? tok : 0) * B + b;
  const uint64_t rowh = (uint64_t)row * H + h;
  float qr[HD], acc[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) { qr[d] = 0.f; acc[d] = 0.f; }
  if (active) {
    load_row<T>(q + row * ldq + h * HD, qr);
#pragma unroll
    for (int d = 0; d < HD; ++d) qr[d] *= scale;
  }
  const uint32_t thr = pdrop > 0.f ? (uint32_t)fminf(pdrop * 4294967296.f, 4294967040.f) : 0u;
  const float inv_keep = pdrop > 0.f ? 1.f / (1.f - pdrop) : 1.f;
  stage_bias(pad, b, Lk, bias);
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < Lk; j0 += CH) {
    const int n = min(CH, Lk - j0), n4 = (n + 3) & ~3;
    if (j0) __syncthreads();                                            // every thread is done with the previous chunk
    stage_chunk<T>(k, ldk, v, ldv, b, B, H, j0, n, n4, ks, vs);
    __syncthreads();
    if (active) {
      for (int j = 0; j < n4; j += 4) {
        const float4 ksc4 = keep_scale4(seed, offset, rowh, j0 + j, thr, inv_keep);
        const float ksc[4] = {ksc4.x, ksc4.y, ksc4.z, ksc4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4* kj = reinterpret_cast<const float4*>(ks + ((j + e) * H + h) * HS);
          float s = bias[j0 + j + e];
#pragma unroll
          for (int d4 = 0; d4 < HD / 4; ++d4) {
            const float4 kk = kj[d4];
            s += qr[4 * d4] * kk.x + qr[4 * d4 + 1] * kk.y + qr[4 * d4 + 2] * kk.z + qr[4 * d4 + 3] * kk.w;
          }
          const float mn = fmaxf(m, s);
          // masked keys (s = -inf) contribute nothing, also while every key so far -- of this and of earlier chunks -- was masked
          // (m = mn = -inf: no inf - inf)
          const float corr = m == -INFINITY ? 0.f : __expf(m - mn), p = s == -INFINITY ? 0.f : __expf(s - mn);
          l = l * corr + p;
          const float pk = p * ksc[e];
          const float4* vj = reinterpret_cast<const float4*>(vs + ((j + e) * H + h) * HS);
#pragma unroll
          for (int d4 = 0; d4 < HD / 4; ++d4) {
            const float4 vv = vj[d4];
            acc[4 * d4] = acc[4 * d4] * corr + pk * vv.x;
            acc[4 * d4 + 1] = acc[4 * d4 + 1] * corr + pk * vv.y;
            acc[4 * d4 + 2] = acc[4 * d4 + 2] * corr + pk * vv.z;
            acc[4 * d4 + 3] = acc[4 * d4 + 3] * corr + pk * vv.w;
          }
          m = mn;
        }
      }
    }
  }
  if (active) {
    const float il = 1.f / l;
    T* o = out + row * ldo + h * HD;
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] = Cvt<T>::from(acc[d] * il);
    lse[rowh] = m + __logf(l);
  }
}

// phase 2 of the backward for chunk CI: thread = (head, channel) adds its share of the group's tokens into the chunk's register sums.
// g2 / q2 point at this thread's channel of the group's first token (row steps sg / sq), pp / dd at its head's parked rows.
template <typename T, int CI, int N>
__device__ __forceinline__ void chunk_sums(float (&accv)[N], float (&acck)[N], const T* __restrict__ g2, const T* __restrict__ q2, long long sg,
                                           long long sq, const float* pp, const float* dd, int H, int part, int nparts, int nt2, int n4) {
  // dout / q of the NEXT token are fetched while this one is summed: the loop is not unrolled, and an L2 round trip per token would
  // otherwise stand in front of every iteration
  float gn = 0.f, qn = 0.f;
  if (part < nt2) { gn = Cvt<T>::to(g2[part * sg]); qn = Cvt<T>::to(q2[part * sq]); }
#pragma unroll 1
  for (int t2 = part; t2 < nt2; t2 += nparts) {
    const float gv = gn, qv = qn;
    if (t2 + nparts < nt2) { gn = Cvt<T>::to(g2[(t2 + nparts) * sg]); qn = Cvt<T>::to(q2[(t2 + nparts) * sq]); }
    const float4* p4p = reinterpret_cast<const float4*>(pp + t2 * H * HS);
    const float4* d4p = reinterpret_cast<const float4*>(dd + t2 * H * HS);
#pragma unroll
    for (int j4 = 0; j4 < CH / 4; ++j4) {
      if (4 * j4 < n4) {                                                 // uniform; blocks past n4 were not parked
        const float4 p4 = p4p[j4], d4 = d4p[j4];
        accv[CI * CH + 4 * j4] += p4.x * gv; accv[CI * CH + 4 * j4 + 1] += p4.y * gv;
        accv[CI * CH + 4 * j4 + 2] += p4.z * gv; accv[CI * CH + 4 * j4 + 3] += p4.w * gv;
        acck[CI * CH + 4 * j4] += d4.x * qv; acck[CI * CH + 4 * j4 + 1] += d4.y * qv;
        acck[CI * CH + 4 * j4 + 2] += d4.z * qv; acck[CI * CH + 4 * j4 + 3] += d4.w * qv;
      }
    }
  }
}

// Backward over the keys of one WINDOW: NCH chunks (1 or 2, compile time: the dK / dV register sums are indexed statically) from key
// `jw` on.  VALU instructions address 256 registers, so sums for more than 64 keys (2 x 64 registers) next to q / dout / dq (96) would
// live in accumulation registers and, at 128 keys, in scratch: past 64 keys the host launches a second window at key 64, whose dq
// share is added to what the first launch wrote (add_dq; same stream, and a (token, head) row belongs to one thread in either launch).
template <typename T, int NCH>
__global__ __launch_bounds__(NT) void attn_longk_bwd(const T* __restrict__ q, long long ldq, const T* __restrict__ k, long long ldk,
                                                     const T* __restrict__ v, long long ldv, const unsigned char* __restrict__ pad,
                                                     const T* __restrict__ dout, long long ldo, const T* __restrict__ out, long long ldout,
                                                     const float* __restrict__ lse, float scale, int Lq, int B, int H, int Lk, float pdrop,
                                                     uint64_t seed, uint64_t offset0, const uint64_t* __restrict__ rng_base,
                                                     int groups_per_block, int jw, int add_dq, T* __restrict__ dq, long long lddq,
                                                     float* __restrict__ dk, float* __restrict__ dv) {
  const uint64_t offset = offset0 + (rng_base ? *rng_base : 0ull);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tok_per = NT / H;
  float* ks = smem;
  float* vs = ks + CH * H * HS;
  float* bias = vs + CH * H * HS;
  float* ps = bias + MAXK;                       // [tok_per][H][HS]  dropped probabilities p~ of the chunk
  float* dss = ps + NT * HS;                     // [tok_per][H][HS]  ds * scale of the chunk
  const int b = blockIdx.y;
  const int tl = threadIdx.x / H, h = threadIdx.x % H;
  const int C = H * HD;
  const uint32_t thr = pdrop > 0.f ? (uint32_t)fminf(pdrop * 4294967296.f, 4294967040.f) : 0u;
  const float inv_keep = pdrop > 0.f ? 1.f / (1.f - pdrop) : 1.f;
  // phase-2 identity of this thread: one channel of one head; NT / C threads share a channel and split the group's tokens
  const int c2 = threadIdx.x % C, part = threadIdx.x / C, nparts = NT / C;
  const int h2 = c2 / HD;
  float accv[NCH * CH], acck[NCH * CH];
#pragma unroll
  for (int j = 0; j < NCH * CH; ++j) accv[j] = acck[j] = 0.f;
  stage_bias(pad, b, Lk, bias);
  float4* pr = reinterpret_cast<float4*>(ps + threadIdx.x * HS);
  float4* dr = reinterpret_cast<float4*>(dss + threadIdx.x * HS);
  for (int g = 0; g < groups_per_block; ++g) {
    const int tok0 = (blockIdx.x * groups_per_block + g) * tok_per;
    if (tok0 >= Lq) break;                                              // uniform
    const int tok = tok0 + tl;
    const bool active = tok < Lq;
    const long long row = (long long)(active ? tok : 0) * B + b;
    const uint64_t rowh = (uint64_t)row * H + h;
    float qr[HD], go[HD], dqr[HD];
    float ls = 0.f, Dsum = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) { qr[d] = 0.f; go[d] = 0.f; dqr[d] = 0.f; }
    if (active) {
      load_row<T>(q + row * ldq + h * HD, qr);
      load_row<T>(dout + row * ldo + h * HD, go);
      const T* o = out + row * ldout + h * HD;
#pragma unroll
      for (int d = 0; d < HD; ++d) Dsum += go[d] * Cvt<T>::to(o[d]);     // D = sum_j p~_j dp~_j = dout . out
      ls = lse[rowh];
    }
#pragma unroll
    for (int wc = 0; wc < NCH; ++wc) {
      const int j0 = jw + wc * CH;
      if (j0 < Lk) {                                                     // uniform
        const int n = min(CH, Lk - j0), n4 = (n + 3) & ~3;
        // (every thread has passed the barrier behind phase 1 of the previous chunk: K / V are free; (p~, ds) are still being read)
        stage_chunk<T>(k, ldk, v, ldv, b, B, H, j0, n, n4, ks, vs);
        __syncthreads();                                                 // K / V (and the bias) staged; phase 2 of the previous chunk done
        if (active) {
#pragma unroll 1
          for (int j = 0; j < n4; j += 4) {
            const float4 ksc4 = keep_scale4(seed, offset, rowh, j0 + j, thr, inv_keep);
            const float ksc[4] = {ksc4.x, ksc4.y, ksc4.z, ksc4.w};
            float pt[4], dsv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float4* kj = reinterpret_cast<const float4*>(ks + ((j + e) * H + h) * HS);
              const float4* vj = reinterpret_cast<const float4*>(vs + ((j + e) * H + h) * HS);
              float s = 0.f, dpt = 0.f;
#pragma unroll
              for (int d4 = 0; d4 < HD / 4; ++d4) {
                const float4 kk = kj[d4], vv = vj[d4];
                s += qr[4 * d4] * kk.x + qr[4 * d4 + 1] * kk.y + qr[4 * d4 + 2] * kk.z + qr[4 * d4 + 3] * kk.w;
                dpt += go[4 * d4] * vv.x + go[4 * d4 + 1] * vv.y + go[4 * d4 + 2] * vv.z + go[4 * d4 + 3] * vv.w;
              }
              const float p = __expf(s * scale + bias[j0 + j + e] - ls);
              const float ds = p * (ksc[e] * dpt - Dsum) * scale;       // ds_j = p_j (dp_j - D), dp_j = keep_j dp~_j
              pt[e] = p * ksc[e];                                       // p~_j: what multiplied v_j in the forward
              dsv[e] = ds;
#pragma unroll
              for (int d4 = 0; d4 < HD / 4; ++d4) {
                const float4 kk = kj[d4];
                dqr[4 * d4] += ds * kk.x; dqr[4 * d4 + 1] += ds * kk.y; dqr[4 * d4 + 2] += ds * kk.z; dqr[4 * d4 + 3] += ds * kk.w;
              }
              __builtin_amdgcn_sched_barrier(0);                          // one key's K / V rows in flight at a time: registers
            }
            pr[j >> 2] = make_float4(pt[0], pt[1], pt[2], pt[3]);
            dr[j >> 2] = make_float4(dsv[0], dsv[1], dsv[2], dsv[3]);
          }
        }
        __syncthreads();
        // phase 2: thread = (head, channel)
        const long long row20 = (long long)tok0 * B + b;
        const int nt2 = min(tok_per, Lq - tok0);                         // tokens past Lq parked nothing and are not visited
        const T* g2p = dout + row20 * ldo + c2;
        const T* q2p = q + row20 * ldq + c2;
        const float* pp = ps + h2 * HS;
        const float* dd = dss + h2 * HS;
        if (wc == 0) chunk_sums<T, 0>(accv, acck, g2p, q2p, (long long)B * ldo, (long long)B * ldq, pp, dd, H, part, nparts, nt2, n4);
        else chunk_sums<T, NCH - 1>(accv, acck, g2p, q2p, (long long)B * ldo, (long long)B * ldq, pp, dd, H, part, nparts, nt2, n4);
      }
    }
    if (active) {
      T* o = dq + row * lddq + h * HD;
      if (add_dq) {
#pragma unroll
        for (int d = 0; d < HD; ++d) dqr[d] += Cvt<T>::to(o[d]);
      }
#pragma unroll
      for (int d = 0; d < HD; ++d) o[d] = Cvt<T>::from(dqr[d]);
    }
  }
#pragma unroll
  for (int j = 0; j < NCH * CH; ++j) {
    if (jw + j < Lk) {
      atomicAdd(dv + ((long long)(jw + j) * B + b) * C + c2, accv[j]);
      atomicAdd(dk + ((long long)(jw + j) * B + b) * C + c2, acck[j]);
    }
  }
}

constexpr size_t CU_LDS = 160 * 1024;

inline int check_dims(int Lq, int B, int H, int hd, int Lk) {
  if (Lq < 0 || B < 0 || H <= 0 || Lk <= 0) return -1006;
  if (hd != HD || H > 8 || (NT % H) != 0 || Lk > MAXK || B > 65535) return -2000;     // shape not served: the caller uses its generic path
  return 0;
}

// kernels that may need more than the default 64-KB dynamic-LDS window opt in once per instantiation
template <typename K>
inline void allow_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

#define FWD_LAUNCH(T_)                                                                                                                    \
  allow_lds(attn_longk_fwd<T_>, lds);                                                                                                     \
  attn_longk_fwd<T_><<<grid, NT, lds, st>>>((const T_*)q, ldq, (const T_*)k, ldk, (const T_*)v, ldv, key_pad, scale, Lq, B, H, Lk, pdrop, seed, \
                                            offset, (const uint64_t*)rng_base, (T_*)out, ldo, lse)

extern "C" int ocpg_attn_longk_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv,
                                   const unsigned char* key_pad, float scale, int Lq, int B, int H, int hd, int Lk, float pdrop,
                                   unsigned long long seed, unsigned long long offset, const unsigned long long* rng_base, void* out,
                                   long long ldo, float* lse, int dtype, void* stream) {
  if (int e = check_dims(Lq, B, H, hd, Lk)) return e;
  if (Lq == 0 || B == 0) return 0;
  if (!q) return -1001;
  if (!k) return -1003;
  if (!v) return -1005;
  if (!out) return -1018;
  if (!lse) return -1020;
  if (dtype < 0 || dtype > 2) return -1021;
  const size_t lds = ((size_t)2 * CH * H * HS + MAXK) * sizeof(float);
  if (lds > CU_LDS) return -2000;
  const int tok_per = NT / H;
  const dim3 grid((unsigned)((Lq + tok_per - 1) / tok_per), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) { FWD_LAUNCH(float); }
  else if (dtype == 1) { FWD_LAUNCH(__hip_bfloat16); }
  else { FWD_LAUNCH(__half); }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

#define BWD_LAUNCH(T_, NCH_, JW_)                                                                                                         \
  allow_lds(attn_longk_bwd<T_, NCH_>, lds);                                                                                               \
  attn_longk_bwd<T_, NCH_><<<grid, NT, lds, st>>>((const T_*)q, ldq, (const T_*)k, ldk, (const T_*)v, ldv, key_pad, (const T_*)dout, ldo,  \
                                                  (const T_*)out, ldout, lse, scale, Lq, B, H, Lk, pdrop, seed, offset,                   \
                                                  (const uint64_t*)rng_base, gpb, JW_, JW_ != 0, (T_*)dq, lddq, dk, dv)
// the window at key 0, then, past 64 keys, the window at key 64
#define BWD_DISPATCH(T_)                                      \
  if (Lk <= CH) { BWD_LAUNCH(T_, 1, 0); }                     \
  else { BWD_LAUNCH(T_, 2, 0); }                              \
  if (Lk > 3 * CH) { BWD_LAUNCH(T_, 2, 2 * CH); }             \
  else if (Lk > 2 * CH) { BWD_LAUNCH(T_, 1, 2 * CH); }

extern "C" int ocpg_attn_longk_bwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv,
                                   const unsigned char* key_pad, const void* dout, long long ldo, const void* out, long long ldout,
                                   const float* lse, float scale, int Lq, int B, int H, int hd, int Lk, float pdrop, unsigned long long seed,
                                   unsigned long long offset, const unsigned long long* rng_base, void* dq, long long lddq, float* dk,
                                   float* dv, int dtype, void* stream) {
  if (int e = check_dims(Lq, B, H, hd, Lk)) return e;
  if (Lq == 0 || B == 0) return 0;
  if (!q) return -1001;
  if (!k) return -1003;
  if (!v) return -1005;
  if (!dout) return -1008;
  if (!out) return -1010;
  if (!lse) return -1012;
  if (!dq) return -1023;
  if (!dk) return -1025;
  if (!dv) return -1026;
  if (dtype < 0 || dtype > 2) return -1027;
  const int tok_per = NT / H;
  const size_t lds = ((size_t)2 * CH * H * HS + MAXK + (size_t)2 * NT * HS) * sizeof(float);
  if (lds > CU_LDS) return -2000;
  const long long groups = (Lq + tok_per - 1) / tok_per;
  // a workgroup adds `gpb` token groups into its register sums before the flush.  One workgroup fits a CU (LDS at H = 8, registers),
  // and the flush is 8 / H atomics per (key, channel) of the window per workgroup whatever gpb is: about one workgroup per CU of the 256,
  // so that the grid runs as one round with the fewest flushes.
  const int gpb = (int)((groups * B + 255) / 256);
  const dim3 grid((unsigned)((groups + gpb - 1) / gpb), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0) { BWD_DISPATCH(float); }
  else if (dtype == 1) { BWD_DISPATCH(__hip_bfloat16); }
  else { BWD_DISPATCH(__half); }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
