// Matrix-core variants of the window-attention kernels (csrc/win_attn_mfma.hip); dispatched from csrc/win_attn.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace ocpg_win_mfma {

bool supported(int N, int head_dim, int dtype);      // bf16 / fp16 storage, head_dim 32, the tiles fit the CU's LDS
int fwd(const void* qkv, const float* biasT, const int* region, float scale, int BW, int NW, int N, int H, void* out, float* lse, int dtype,
        hipStream_t st);

// dS: [BW, H, N, N] in the storage dtype, (key, query) order, fully written -- the caller sums it over BW for the bias gradient
// (NULL: the bias needs no gradient)
int bwd(const void* qkv, const float* bias, const float* biasT, const int* region, float scale, int BW, int NW, int N, int H, const void* out,
        const void* dout, const float* lse, void* dqkv, float* Dbuf, void* dS, int dtype, hipStream_t st);

// Opt-in variant: the relative-position TABLE gradient instead of dS.  Table row of (q, key) = tok_code[q] - tok_code[key] + code_off, in
// [0, T); partials [BW, H, T] fp32 workspace and dtable [T, H] fp32 are fully written (nothing to zero).  supported_dtable: the LDS also
// holds the N codes and the T floats.
bool supported_dtable(int N, int head_dim, int dtype, int T);
int bwd_dtable(const void* qkv, const float* bias, const float* biasT, const int* region, float scale, int BW, int NW, int N, int H,
               const void* out, const void* dout, const float* lse, void* dqkv, float* Dbuf, const int* tok_code, int code_off, int T,
               float* partials, float* dtable, int dtype, hipStream_t st);

}  // namespace ocpg_win_mfma
