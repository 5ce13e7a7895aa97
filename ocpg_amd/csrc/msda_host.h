// Host-side pieces of the MSDeformAttn backward shared by the fp32 entry points (msda.hip) and the 16-bit-storage ones (msda_h16.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ocpg_msda {

// grad_value (+=) of the self-attention shape (Lq == S, host shapes given) through the column scatter / output-tiled kernels, with the
// call site's path selection when sel_state is not null (include/ocpg_hip.h: ocpg_msda_bwd_value_sel_f32).
// go_dtype: storage of grad_out, 0 = float32, 1 = bfloat16, 2 = float16.  Forced paths (OCPG_MSDA_TILE / OCPG_MSDA_COL / OCPG_MSDA_COL_LP)
// are honoured as documented there; the single-level column scatter that OCPG_MSDA_COL_LP < 4 forces reads float32 only.
// 0 = launched, -2000 = not served and NOTHING launched, other negatives = a kernel family refused after the geometry checks.
int bwd_value_sel(const float* loc, const float* attn, const void* grad_out, int go_dtype, int N, int S, int M, int D, int L, int Lq, int P,
                  float* grad_value, const int64_t* shapes_host, int* sel_state, hipStream_t st);

}  // namespace ocpg_msda
