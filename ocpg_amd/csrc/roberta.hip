// Forward of the frozen RoBERTa text encoder, the parts the library had no kernel for.  fp32 storage, fp32
// arithmetic, forward only; the dense products stay with ocpg_small_linear_f32_fwd / ocpg_gemm and the residual LayerNorms with
// ocpg_dropout_add_ln_fwd at p = 0.
//
//   ocpg_roberta_embed_ln_f32   out[b, l] = LN(word[ids[b, l]] + type[0] + pos[position(b, l)])
//     ONE WAVE PER TOKEN, four tokens per workgroup.  A row of C <= 1024 channels is at most 4 float4 per lane, so the row stays in
//     registers between the two LayerNorm passes and every reduction is a 6-step wave shuffle: no LDS and no barrier anywhere.  The
//     position id is formed by the token's own wave: it walks the ids of its row 64 at a time up to its own position, ballots
//     "id != pad", popcounts, and carries the count from one 64-lane group to the next.  L is at most P - pad - 1 (a few hundred), so the
//     walk is at most a handful of ballots, cheaper than a second launch with a scan.
//
//   ocpg_attn_hd64_fwd_f32      out = softmax(q k^T scale + mask) v per (batch, head), head_dim 64, 1..128 keys
//     ONE WAVE PER QUERY ROW; the 64 lanes are the KEYS while the scores are formed (lane j owns keys j and j + 64: a 64-term dot over
//     K's row j in LDS, row stride 65 floats, so the 64 lanes read 64 different banks) and the CHANNELS while the output is formed (lane d
//     owns channel d: sum_j p_j V[j][d], V's row j is read by the 64 lanes as 256 contiguous bytes, p_j is an LDS broadcast).  The
//     softmax between the two is two wave reductions over at most two values per lane.  A workgroup is 4 waves and serves QB = 16
//     queries of one (batch, head), 4 per wave, so the grid is H x B x ceil(L / 16): at the 10-20 tokens of a caption the kernel is
//     latency-bound, 12 heads x 2 query blocks put 24 workgroups on 24 CUs, and each stages only L x 64 x 2 floats of K and V (10 KB at
//     L = 20; 70 KB at L = 128, where 8 query blocks re-read the (batch, head)'s K / V from L2).  A mapping with a thread per query would
//     leave 44-54 of 64 lanes idle at those lengths; MFMA tiles of 32 x 32 would be mostly padding.
//
//   ocpg_bias_act_f32           y = act(x + bias), act none / exact GELU / tanh, in place or not, float4 where the addresses allow
//
// Every kernel early-outs by predication only: all threads of a workgroup reach every barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int NT = 256, WAVES = 4;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- embeddings + LayerNorm
constexpr int EMB_NCH = 4;      // float4 per lane: C <= 64 * 4 * 4

__global__ __launch_bounds__(NT) void roberta_embed_ln(const long long* __restrict__ ids, const float* __restrict__ word,
                                                       const float* __restrict__ pos, const float* __restrict__ type0,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int pad_id,
                                                       int B, int L, int C, int V, int P, float* __restrict__ out, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long tok = (long long)blockIdx.x * WAVES + wave;
  const bool live = tok < (long long)B * L;                  // wave-uniform
  const int b = live ? (int)(tok / L) : 0, l = live ? (int)(tok % L) : 0;
  const long long* row = ids + (long long)b * L;
  // position id: pad + #{j <= l : ids[b, j] != pad}, or pad at a pad token
  int count = 0;
  for (int j0 = 0; j0 <= l; j0 += 64) {                      // the carry over the 64-lane groups
    const int j = j0 + lane;
    const bool nonpad = live && j <= l && row[j] != (long long)pad_id;
    count += __popcll(__ballot(nonpad));
  }
  const long long id = live ? row[l] : 0;
  int position = id != (long long)pad_id ? pad_id + count : pad_id;
  position = min(max(position, 0), P - 1);                   // the entry guarantees the range; the clamp costs two instructions
  const bool id_ok = id >= 0 && id < (long long)V;
  if (live && !id_ok && lane == 0 && bad) atomicAdd(bad, 1);
  const int c4 = C >> 2;
  const float4* wrow = reinterpret_cast<const float4*>(word + (id_ok ? id : 0) * (long long)C);
  const float4* prow = reinterpret_cast<const float4*>(pos + (long long)position * C);
  const float4* trow = reinterpret_cast<const float4*>(type0);
  float4 z[EMB_NCH];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < EMB_NCH; ++u) {
    const int i = lane + 64 * u;
    z[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && i < c4) {
      const float4 w = id_ok ? wrow[i] : make_float4(0.f, 0.f, 0.f, 0.f), t = trow[i], p = prow[i];
      z[u] = make_float4((w.x + t.x) + p.x, (w.y + t.y) + p.y, (w.z + t.z) + p.z, (w.w + t.w) + p.w);
      s += (z[u].x + z[u].y) + (z[u].z + z[u].w);
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < EMB_NCH; ++u) {
    if (lane + 64 * u < c4) {
      const float dx = z[u].x - mean, dy = z[u].y - mean, dz = z[u].z - mean, dw = z[u].w - mean;
      q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
  float4* orow = reinterpret_cast<float4*>(out + tok * C);
#pragma unroll
  for (int u = 0; u < EMB_NCH; ++u) {
    const int i = lane + 64 * u;
    if (live && i < c4) {
      const float4 g = reinterpret_cast<const float4*>(gamma)[i], bt = reinterpret_cast<const float4*>(beta)[i];
      orow[i] = make_float4((z[u].x - mean) * rstd * g.x + bt.x, (z[u].y - mean) * rstd * g.y + bt.y, (z[u].z - mean) * rstd * g.z + bt.z,
                            (z[u].w - mean) * rstd * g.w + bt.w);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ attention, head 64
constexpr int HD = 64, KS = HD + 1, VS = HD + 4, QB = 16, QPW = QB / WAVES, MAXL = 128;

template <typename M>
__global__ __launch_bounds__(NT) void attn_hd64_fwd(const float* __restrict__ qkv, const M* __restrict__ attend, float scale, int B, int L, int H,
                                                    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* vs = smem;                       // [L][VS]   (first: float4-aligned rows)
  float* ks = vs + L * VS;                // [L][KS]
  float* qs = ks + L * KS;                // [WAVES][HD]
  float* ps = qs + WAVES * HD;            // [WAVES][MAXL]
  const int h = blockIdx.x, b = blockIdx.y, q0 = blockIdx.z * QB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long tok_stride = 3LL * H * HD;
  const float* base = qkv + (long long)b * L * tok_stride + (long long)h * HD;
  // stage K and V of the (batch, head): 16 float4 per row and matrix
  for (int i = threadIdx.x; i < L * (HD / 4); i += NT) {
    const int j = i >> 4, c = (i & 15) * 4;
    const float4 kv = *reinterpret_cast<const float4*>(base + j * tok_stride + (long long)H * HD + c);
    const float4 vv = *reinterpret_cast<const float4*>(base + j * tok_stride + 2LL * H * HD + c);
    float* kd = ks + j * KS + c;
    kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
    *reinterpret_cast<float4*>(vs + j * VS + c) = vv;
  }
  // the two keys of this lane
  const int j0 = lane, j1 = lane + 64;
  const bool on0 = j0 < L && attend[(long long)b * L + (j0 < L ? j0 : 0)] != 0;
  const bool on1 = j1 < L && attend[(long long)b * L + (j1 < L ? j1 : 0)] != 0;
  const float* k0 = ks + (j0 < L ? j0 : 0) * KS;
  const float* k1 = ks + (j1 < L ? j1 : 0) * KS;
  float* myq = qs + wave * HD;
  float* myp = ps + wave * MAXL;
  for (int t = 0; t < QPW; ++t) {                                       // the same trip count in every wave: barriers inside
    const int qi = q0 + t * WAVES + wave;
    const bool live = qi < L;                                            // wave-uniform
    myq[lane] = live ? base[qi * tok_stride + lane] : 0.f;
    __syncthreads();                                                     // K / V staged (t = 0), this wave's q visible
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 16
    for (int d = 0; d < HD; ++d) {
      const float qd = myq[d];
      s0 = fmaf(qd, k0[d], s0);
      s1 = fmaf(qd, k1[d], s1);
    }
    s0 = on0 ? s0 * scale : -INFINITY;
    s1 = on1 ? s1 * scale : -INFINITY;
    float m = wave_max(fmaxf(s0, s1));
    if (m == -INFINITY) m = 0.f;                                         // a row without an attended key (outside the contract): zeros, no NaN
    const float p0 = on0 ? __expf(s0 - m) : 0.f, p1 = on1 ? __expf(s1 - m) : 0.f;
    const float lsum = wave_sum(p0 + p1);
    myp[j0] = p0;
    myp[j1] = p1;
    __syncthreads();
    float acc = 0.f;
    for (int j = 0; j < L; ++j) acc = fmaf(myp[j], vs[j * VS + lane], acc);
    if (live) out[((long long)b * L + qi) * ((long long)H * HD) + (long long)h * HD + lane] = lsum > 0.f ? acc / lsum : 0.f;
    __syncthreads();                                                     // myq / myp are rewritten by the next query
  }
}

// ------------------------------------------------------------------------------------------------------------- bias + activation
__device__ __forceinline__ float act_f(float v, int act) {
  if (act == 1) return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
  if (act == 2) return tanhf(v);
  return v;
}

// y may alias x: every element is read and written by one thread only (no __restrict__ on x / y)
__global__ __launch_bounds__(NT) void bias_act(const float* x, const float* __restrict__ bias, long long n, int C, int act, int vec, float* y) {
  const long long stride = (long long)gridDim.x * NT;
  const long long n4 = vec ? n >> 2 : 0;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    int c = (int)((i * 4) % C);
    float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[e] = act_f(r[e] + (bias ? bias[c] : 0.f), act);
      c = c + 1 == C ? 0 : c + 1;
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(r[0], r[1], r[2], r[3]);
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * NT + threadIdx.x; i < n; i += stride)
    y[i] = act_f(x[i] + (bias ? bias[i % C] : 0.f), act);
}

inline int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

template <typename K>
inline void allow_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int ocpg_roberta_embed_ln_f32(const long long* ids, const float* word, const float* pos, const float* type0, const float* gamma,
                              const float* beta, float eps, int pad_id, int B, int L, int C, int V, int P, float* out, int* bad, void* stream) {
  if (B < 0 || L < 0 || C <= 0 || V <= 0 || P <= 0 || pad_id < 0) return -1009;
  if (C % 4 != 0 || C > 64 * 4 * EMB_NCH) return -2000;
  if ((long long)L + pad_id + 1 > P) return -2501;                 // a row of L non-pad tokens would read past the position table
  if (B == 0 || L == 0) return 0;
  if (!ids) return -1001;
  if (!word || !aligned16(word)) return -1002;
  if (!pos || !aligned16(pos)) return -1003;
  if (!type0 || !aligned16(type0)) return -1004;
  if (!gamma || !aligned16(gamma)) return -1005;
  if (!beta || !aligned16(beta)) return -1006;
  if (!out || !aligned16(out)) return -1014;
  const long long tokens = (long long)B * L, blocks = (tokens + WAVES - 1) / WAVES;
  if (blocks > 0x7fffffffLL) return -1009;
  roberta_embed_ln<<<(unsigned)blocks, NT, 0, (hipStream_t)stream>>>(ids, word, pos, type0, gamma, beta, eps, pad_id, B, L, C, V, P, out, bad);
  return status();
}

int ocpg_attn_hd64_fwd_f32(const float* qkv, const void* attend, int attend_i64, float scale, int B, int L, int H, float* out, void* stream) {
  if (B < 0 || L < 0 || H < 0) return -1005;
  if (attend_i64 != 0 && attend_i64 != 1) return -1003;
  if (L < 1 || L > MAXL || H < 1 || H > 65535 || B > 65535) return -2000;
  if (B == 0) return 0;
  if (!qkv || !aligned16(qkv)) return -1001;
  if (!attend) return -1002;
  if (!out) return -1008;
  const size_t lds = sizeof(float) * ((size_t)L * (KS + VS) + WAVES * HD + WAVES * MAXL);
  const dim3 grid(H, B, (L + QB - 1) / QB);
  if (attend_i64) {
    allow_lds(attn_hd64_fwd<long long>, lds);
    attn_hd64_fwd<long long><<<grid, NT, lds, (hipStream_t)stream>>>(qkv, (const long long*)attend, scale, B, L, H, out);
  } else {
    allow_lds(attn_hd64_fwd<unsigned char>, lds);
    attn_hd64_fwd<unsigned char><<<grid, NT, lds, (hipStream_t)stream>>>(qkv, (const unsigned char*)attend, scale, B, L, H, out);
  }
  return status();
}

int ocpg_bias_act_f32(const float* x, const float* bias, long long R, int C, int act, float* y, void* stream) {
  if (R < 0 || C <= 0) return -1003;
  if (act < 0 || act > 2) return -1005;
  if (R == 0) return 0;
  if (!x) return -1001;
  if (!y) return -1006;
  const long long n = R * C;
  const int vec = aligned16(x) && aligned16(y);
  const long long work = vec ? (n + 3) / 4 : n;
  long long blocks = (work + NT - 1) / NT;
  if (blocks > 2048) blocks = 2048;
  bias_act<<<(unsigned)blocks, NT, 0, (hipStream_t)stream>>>(x, bias, n, C, act, vec, y);
  return status();
}

}  // extern "C"
