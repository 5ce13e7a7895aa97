// The LFM block's two Fourier transforms for EVERY line length 1 <= L <= 256 (csrc/lfm_dft.hip serves L = L1 * L2, both <= 16, L <= 128;
// a map it refuses -- a multiple of a prime >= 17, 125, anything above 128 -- took the library FFT between two transposing copies).
// The same four passes with the same contracts (see the head of lfm_dft.hip): rows_fwd, cols_fwd (gate, norm, Hermitian mirror, [Re || Im]
// pair in fp32 / bf16 / fp16), cols_inv (gate, Hermitian part, partial sums of the coefficient gradient), rows_inv (norm, .real,
// residual); channels-last maps, a lane owns ONE CHANNEL of a line, half spectrum along w, fp32 arithmetic, no atomics, no memset, two
// launches per direction with every size passed by value.  lfm_dft.hip is untouched and shares no code with this file.
//
// A line transform follows a PLAN of up to three stages (r1, r2, r3; product L; a stage of 1 is skipped), decimation in time, in place in
// an LDS tile [L][CHW channels] of float2.  With the stages that are not 1 called s0, s1, s2: stage i has P = the product of the stages
// before it, R = s_i, Q = the product of the stages after it; it runs P * Q independent DFTs of length R -- batch (kp, jr), kp < P, jr < Q,
// over slots kp R Q + j Q + jr (j < R), output k left in slot kp R Q + k Q + jr and multiplied by W_L^(P jr k) when Q > 1.  After the
// last stage spectrum element k = k0 + s0 k1 + s0 s1 k2 sits in slot (k0 s1 + k1) s2 + k2; the epilogues read that from a table.
//   * a stage R <= 16 is the kind lfm_dft.hip has: a wave takes a batch, a lane keeps its R inputs in registers, the R x R DFT matrix is
//     read row by row with wave-uniform (scalar) loads.
//   * a stage R = p, ONE prime 17 <= p <= 251 (every L <= 256 that is not 16-smooth is p * m with m <= 15): the direct O(p^2) transform.
//     p inputs do not fit in registers, so they are read from the tile; a wave holds NU units of 8 consecutive outputs of a batch in
//     registers (NW * NU * 8 >= p: a batch never spans a round), all waves meet at a barrier and only then write the outputs over the
//     batch's inputs.  W_p^(jk) = W_L^((L/p) (jk mod p)) comes from the table of W_L powers; the INDEX is carried by add-and-wrap
//     recurrences (never the value), wave-uniform, so the twiddles are scalar loads.  The plan puts p LAST: along w the forward pass then
//     computes only the half spectrum's outputs (kmax) and the inverse pass only real parts (REAL_OUT) in the expensive stage; a real
//     input (REAL_IN) halves it where p is the only stage.
// LDS: the tile stays within the 64 KB lfm_dft.hip uses: L <= 128 takes 64 channels per workgroup (256 threads, 4 waves), 129..256 takes
// 32 channels (512 threads, 8 waves).  In the 32-channel form lanes 32..63 of a wave are IDLE in the stages (a second line would need a
// second tile) and work in the prologues / epilogues, where a thread's element index is threadIdx.x / CHW.
#include "lfm_dft_any_kernel.h"

extern "C" {

int ocpg_lfm_spectrum_fwd_any(const float* x, const float* coef, const float* high, int N, int H, int W, int C, const void* tw_h, const void* tw_w,
                              float norm, void* tmp, void* pair, int pair_dt, int h1, int h2, int h3, int w1, int w2, int w3, void* stream) {
  if (N < 0 || H < 1 || W < 1 || C < 1) return -1003;
  if (N == 0) return 0;
  const Plan ph = plan_of(H, h1, h2, h3), pw = plan_of(W, w1, w2, w3);
  if (!ph.L || !pw.L) return -2000;
  if (!x) return -1001;
  if (!tw_h || !tw_w) return -1005;
  if (!tmp) return -1011;
  if (!pair) return -1012;
  if ((coef == nullptr) != (high == nullptr)) return -1002;
  if (pair_dt < 0 || pair_dt > 2) return -1013;
  hipStream_t st = (hipStream_t)stream;
  const int Wh = W / 2 + 1;
  if ((long long)N * H > 2147483647LL || (long long)N * Wh > 2147483647LL) return -1003;
  if (chw_of(W) == 64)
    rows_fwd_any<64><<<dim3((unsigned)(N * H), (C + 63) / 64), 256, (size_t)W * 64 * sizeof(float2), st>>>(x, W, C, pw, (const float2*)tw_w, (float2*)tmp);
  else
    rows_fwd_any<32><<<dim3((unsigned)(N * H), (C + 31) / 32), 512, (size_t)W * 32 * sizeof(float2), st>>>(x, W, C, pw, (const float2*)tw_w, (float2*)tmp);
  if (chw_of(H) == 64) {
    if (pair_dt == 0) launch_cols_fwd<64, float>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else if (pair_dt == 1) launch_cols_fwd<64, __hip_bfloat16>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else launch_cols_fwd<64, __half>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
  } else {
    if (pair_dt == 0) launch_cols_fwd<32, float>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else if (pair_dt == 1) launch_cols_fwd<32, __hip_bfloat16>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
    else launch_cols_fwd<32, __half>(tmp, coef, high, N, H, W, C, ph, tw_h, norm, pair, st);
  }
  return status();
}

int ocpg_lfm_spectrum_inv_any(const void* pair, int pair_dt, const float* coef, const float* high, const void* z_saved, float* coef_part, int N, int H,
                              int W, int C, const void* tw_h, const void* tw_w, float norm, void* tmp, const float* residual, float* out, int h1, int h2,
                              int h3, int w1, int w2, int w3, void* stream) {
  if (N < 0 || H < 1 || W < 1 || C < 1) return -1007;
  if (N == 0) return 0;
  const Plan ph = plan_of(H, h1, h2, h3), pw = plan_of(W, w1, w2, w3);
  if (!ph.L || !pw.L) return -2000;
  if (!pair) return -1001;
  if (!tw_h || !tw_w) return -1011;
  if (!tmp) return -1014;
  if (!out) return -1016;
  if ((coef == nullptr) != (high == nullptr)) return -1003;
  if (coef_part && (!coef || !z_saved)) return -1005;
  if (pair_dt < 0 || pair_dt > 2) return -1002;
  hipStream_t st = (hipStream_t)stream;
  const int Wh = W / 2 + 1;
  if ((long long)N * H > 2147483647LL || (long long)N * Wh > 2147483647LL) return -1007;
  if (chw_of(H) == 64) {
    if (pair_dt == 0) launch_cols_inv<64, float>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else if (pair_dt == 1) launch_cols_inv<64, __hip_bfloat16>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else launch_cols_inv<64, __half>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
  } else {
    if (pair_dt == 0) launch_cols_inv<32, float>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else if (pair_dt == 1) launch_cols_inv<32, __hip_bfloat16>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
    else launch_cols_inv<32, __half>(pair, coef, high, z_saved, coef_part, N, H, W, C, ph, tw_h, tmp, st);
  }
  if (chw_of(W) == 64)
    rows_inv_any<64><<<dim3((unsigned)(N * H), (C + 63) / 64), 256, (size_t)W * 64 * sizeof(float2), st>>>((const float2*)tmp, W, C, pw, (const float2*)tw_w, norm,
                                                                                                        residual, out);
  else
    rows_inv_any<32><<<dim3((unsigned)(N * H), (C + 31) / 32), 512, (size_t)W * 32 * sizeof(float2), st>>>((const float2*)tmp, W, C, pw, (const float2*)tw_w, norm,
                                                                                                        residual, out);
  return status();
}

}  // extern "C"
