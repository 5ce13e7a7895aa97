/* libocpg_hip.so -- C ABI of the MI355X (gfx950) kernels behind OCPG's per-clip hot path.
 *
 * Drop-in boundary #2 of SURVEY.md section 8b.  The reference binds its native op through the pybind11
 * module `MultiScaleDeformableAttention` (models/ops/src/vision.cpp:13-16) whose two entry points are
 * declared in models/ops/src/ms_deform_attn.h:20-61 and implemented for CUDA in
 * models/ops/src/cuda/ms_deform_attn_cuda.cu:20-80 (forward) and :83-152 (backward).  The functions below
 * are what a ctypes / pybind stub for that path binds instead.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes, no torch types; every tensor contiguous, row-major, same device;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); launches are asynchronous.  The KERNEL entry points
 *     neither synchronise nor allocate.  ONE exception, the GEMM family (ocpg_gemm, ocpg_gemm_bn_act: csrc/gemm.hip): it keeps a
 *     per-device PLAN CACHE (mutex-protected) and, at the FIRST use of a (device, stream) pair / of a plan, hipMallocs a hipBLASLt
 *     workspace and -- with OCPG_GEMM_TUNE=1, the default -- scratch outputs to time the heuristic's candidates, synchronising on
 *     its own events while it does.  Consequences for callers: run one un-captured call per shape and stream before capturing a
 *     HIP graph (bench.py's warm-up steps on the capture stream); OCPG_GEMM_TUNE=0 pins the heuristic's first choice
 *     (run-to-run and rank-to-rank reproducible kernel selection);
 *   - return 0 on success, a negative hipError_t on a launch/runtime error, -1000-k for the k-th
 *     argument being invalid (null pointer / non-positive size);
 *   - outputs are caller-allocated.  Forward outputs are fully overwritten.  In the backward,
 *     grad_value is ACCUMULATED into (scatter-add): the caller zeroes it first, exactly as
 *     ms_deform_attn_cuda.cu:121 does with at::zeros_like; grad_loc / grad_attn are fully overwritten;
 *   - re-entrant and thread-safe; no global state except the GEMM plan cache above (and, in diagnostic builds only, the
 *     EXP_STAMPS counters of the halo-staged 3x3 convolution).
 *
 * Tensor contract of MSDeformAttn (ms_deform_attn_cuda.cu:28-48):
 *   value        [N, S, M, D]          S = sum_l H_l*W_l
 *   shapes       [L, 2]  int64 (H, W)   device memory  (+ optional host copy, see below)
 *   level_start  [L]     int64          device memory
 *   loc          [N, Lq, M, L, P, 2]    (x, y) normalised to [0,1]
 *   attn         [N, Lq, M, L, P]
 *   out / grad_out [N, Lq, M*D]
 * Unlike the reference there is no im2col_step chunking and therefore no `N % im2col_step == 0`
 * restriction (ms_deform_attn_cuda.cu:50-52); any N works.
 */
#ifndef OCPG_HIP_H
#define OCPG_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* replaces ms_deform_attn_forward (ms_deform_attn.h:20-39 -> ms_deform_attn_cuda.cu:20-80), float32.
 * shapes_host: optional HOST copy of `shapes` (may be NULL).  When given, Lq == S (self-attention over the value's
 * own pixels, the encoder case: query q IS pixel q) and level_start is the exclusive prefix sum of H_l*W_l, the
 * column-tile kernels (LDS-staged sampling windows) are selected; results are identical either way up to fp32
 * summation order.  The host copy is what the reference's module already owns: ms_deform_attn.py:94 asserts on the
 * same tensor, which reads it back to the host on every call. */
int ocpg_msda_fwd_f32(const float* value, const int64_t* shapes, const int64_t* level_start,
                      const float* loc, const float* attn,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      float* out, const int64_t* shapes_host, void* stream);
/* float64 variant (AT_DISPATCH_FLOATING_TYPES, ms_deform_attn_cuda.cu:64); used by the test.py protocol */
int ocpg_msda_fwd_f64(const double* value, const int64_t* shapes, const int64_t* level_start,
                      const double* loc, const double* attn,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      double* out, void* stream);

/* replaces ms_deform_attn_backward (ms_deform_attn.h:41-61 -> ms_deform_attn_cuda.cu:83-152), float32.
 * shapes_host: as for the forward (may be NULL): selects the column-tile backward (gather kernel for grad_loc /
 * grad_attn + bin-and-sum scatter kernel for grad_value) when Lq == S and the column scatter serves the shape (D = 16 or 32, a
 * P and level count its geometry takes, OCPG_MSDA_COL not 0).  Every other call -- NULL, Lq != S, D = 64, ... -- runs the row
 * kernel that gathers and scatters with fp32 atomics in one launch (D = 4 * 2^k <= 256), or the generic kernel (any D). */
int ocpg_msda_bwd_f32(const float* value, const int64_t* shapes, const int64_t* level_start,
                      const float* loc, const float* attn, const float* grad_out,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      float* grad_value, float* grad_loc, float* grad_attn,
                      const int64_t* shapes_host, void* stream);
/* The two independent halves of ocpg_msda_bwd_f32 on their own (same contract; return -2000 when the shape is not
 * served by the dedicated kernel -- call ocpg_msda_bwd_f32 then).  A caller that needs only some of the gradients
 * (ctx.needs_input_grad of ms_deform_attn_func.py:30-39), or that wants the two kernels timed separately, binds these:
 *   _value:   grad_value (+=) from loc / attn / grad_out alone (column-tile bin-and-sum scatter; needs shapes_host, Lq == S)
 *   _locattn: grad_loc and grad_attn (overwritten) -- gather-only row kernel, any Lq */
int ocpg_msda_bwd_value_f32(const float* loc, const float* attn, const float* grad_out,
                            int N, int S, int M, int D, int L, int Lq, int P,
                            float* grad_value, const int64_t* shapes_host, void* stream);
int ocpg_msda_bwd_locattn_f32(const float* value, const int64_t* shapes, const int64_t* level_start,
                              const float* loc, const float* attn, const float* grad_out,
                              int N, int S, int M, int D, int L, int Lq, int P,
                              float* grad_loc, float* grad_attn, void* stream);
/* ocpg_msda_bwd_value_f32 with PER-CALL PATH SELECTION (round 4; replaces the same reference kernel, cuh:301-403 via cu:83-152, for
 * grad_value).  Two kernel families serve the self-attention shape: the query-owned column scatter (fastest while the offsets stay
 * within ~5 pixels of the query, as at initialisation) and the output-tiled kernels (no halo atomics: ahead once training has spread
 * the offsets).  sel_state: 8 ints of device memory (8-byte aligned: slots 0 / 1 are one 64-bit word the reporting workgroups add to)
 * owned by the CALL SITE (one per MSDeformAttn module), zero-filled once and passed
 * to every call; the kernels keep in it the share of samples that missed the active path's locality assumption and the path the next
 * call takes (0 = column, 1 = tiled; slots 6 / 7: far and total samples of the last call, for diagnostics).  Both families are launched
 * on every call and the inactive one's workgroups return at once, so the choice needs no host round trip and survives HIP-graph replay.
 * NULL state, a shape one of the families does not serve, or a forced path (OCPG_MSDA_TILE / OCPG_MSDA_COL): as ocpg_msda_bwd_value_f32. */
/* FUSED FRONT END of the MSDeformAttn module (round 4).  Replaces, for self-attention calls with 2-d reference points, the elementwise
 * passes of models/ops/modules/ms_deform_attn.py:96-110 around the op: softmax over the L*P attention logits, `reference + offset`, and in
 * the backward the softmax gradient and the concatenation of the offset / logit gradients.
 *   qproj [N*Lq, 3*M*L*P]  the merged query projection: columns [0, 2*M*L*P) = sampling offsets (M, L, P, 2) ALREADY divided by (W_l, H_l)
 *                          (the caller folds that division into the projection's weight rows), columns [2*M*L*P, 3*M*L*P) = logits (M, L*P)
 *   ref   [N*Lq, L, 2]     reference points (x, y), normalised
 *   _fwd:       out [N, Lq, M*D] as ocpg_msda_fwd_f32, plus the sampling locations loc_out [N, Lq, M, L, P, 2] and the attention weights
 *               attn_out [N, Lq, M, L, P] it derived (the module returns them; the backward entry points below read them)
 *   _bwd_qproj: grad_qproj [N*Lq, 3*M*L*P] (overwritten) = [d offsets | d logits] from value / loc / attn / grad_out -- the gather half of
 *               the backward (ocpg_msda_bwd_locattn_f32) with the softmax backward in its epilogue; grad_value comes from
 *               ocpg_msda_bwd_value_f32 / _sel_f32 as before.
 * D = 32 and L*P = 16 only; -2000 otherwise (nothing launched: keep the unfused path). */
int ocpg_msda_fused_fwd_f32(const float* value, const int64_t* shapes, const int64_t* level_start,
                            const float* qproj, const float* ref,
                            int N, int S, int M, int D, int L, int Lq, int P,
                            float* out, float* loc_out, float* attn_out, void* stream);
int ocpg_msda_fused_bwd_qproj_f32(const float* value, const int64_t* shapes, const int64_t* level_start,
                                  const float* loc, const float* attn, const float* grad_out,
                                  int N, int S, int M, int D, int L, int Lq, int P,
                                  float* grad_qproj, void* stream);
int ocpg_msda_bwd_value_sel_f32(const float* loc, const float* attn, const float* grad_out,
                                int N, int S, int M, int D, int L, int Lq, int P,
                                float* grad_value, const int64_t* shapes_host, int* sel_state, void* stream);
int ocpg_msda_bwd_f64(const double* value, const int64_t* shapes, const int64_t* level_start,
                      const double* loc, const double* attn, const double* grad_out,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      double* grad_value, double* grad_loc, double* grad_attn, void* stream);

/* SAMPLE FIRST, PROJECT AFTERWARDS (csrc/msda_sample_first.hip): the module's value_proj + padding fill + op for calls with few queries
 * (cross-attention: Lq << S), float32.  Sampling is linear in value and value_proj is the same map for every token, so
 *   out[n, q, h*D..] = s[n, q, h, :] . Wv[h*D.., :]^T + beta[n, q, h] * bv[h*D..]
 * with s = the attention-weighted bilinear sample of the UNPROJECTED tokens and beta = the sum of the weights that went into it.  The
 * result is what F.linear -> masked_fill -> ocpg_msda_fwd_f32 gives, up to fp32 summation order; value [N, S, M, D] is never formed.
 *   src [N, S, C] (C = M * D), wv [C, C] (row = output channel), bv [C] or NULL, pad [N, S] bytes (non-zero = padded token) or NULL,
 *   shapes / level_start / loc / attn as for ocpg_msda_fwd_f32.
 *   _fwd:        out [N, Lq, C]; s [N, Lq, M, C] and beta [N, Lq, M] are written for the backward.
 *   _bwd:        grad_src [N, S, C] is ACCUMULATED into by float atomics (the caller zeroes it, as grad_value of ocpg_msda_bwd_f32; NULL =
 *                not wanted); grad_loc / grad_attn are overwritten.
 *   _bwd_params: grad_wv [C, C] and grad_bv [C] (NULL = not wanted) from grad_out, s and beta: overwritten, fixed summation order.
 * Served: C % 64 == 0, C <= 1024, L * P <= 64, S * C < 2^31, naturally aligned buffers; anything else returns -2000 with nothing
 * launched (alignment included: it is examined before the first launch) and the caller keeps value_proj + ocpg_msda_fwd_f32 / _bwd_f32. */
int ocpg_msda_sf_fwd_f32(const float* src, const float* wv, const float* bv, const unsigned char* pad,
                         const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                         int N, int S, int M, int D, int L, int Lq, int P,
                         float* out, float* s, float* beta, void* stream);
int ocpg_msda_sf_bwd_f32(const float* src, const float* wv, const float* bv, const unsigned char* pad,
                         const int64_t* shapes, const int64_t* level_start, const float* loc, const float* attn,
                         const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                         float* grad_src, float* grad_loc, float* grad_attn, void* stream);
int ocpg_msda_sf_bwd_params_f32(const float* grad_out, const float* s, const float* beta, int N, int M, int D, int Lq,
                                float* grad_wv, float* grad_bv, void* stream);

/* MSDeformAttn with 16-BIT STORAGE of value / out / grad_out (opt-in; the reference's op is fp32 / fp64 only, so these entry points
 * have no counterpart there and the parity statement does not cover them).
 *   dtype: 1 = bfloat16, 2 = float16 (the numbering of ocpg_bn_act_*: 0 would be float32 -- use the _f32 entry points); any other
 *          value returns an invalid-argument status and launches nothing.
 *   value [N, S, M, D], out / grad_out [N, Lq, M*D]: 16-bit elements of `dtype`.
 *   loc, attn, grad_loc, grad_attn: float32 (a normalised coordinate on an 80-wide map does not survive 8 mantissa bits).
 *   grad_value [N, S, M, D]: float32, ACCUMULATED into (caller zeroes it), exactly as ocpg_msda_bwd_f32 -- there are no 16-bit atomics.
 *   Arithmetic is fp32 throughout; every 16-bit element is widened exactly at its load and `out` is rounded to nearest-even once, at
 *   its store.  With value' = value widened to fp32 (exact), _fwd_h16 returns round(ocpg_msda_fwd_f32(value')) up to fp32 summation
 *   order, and _bwd_h16 the gradients ocpg_msda_bwd_f32(value', grad_out') gives, up to fp32 summation order.
 *   Any D is served; D % 4 == 0 (D / 4 a power of two <= 64) takes the fast row kernels when value / out / grad_out are 16-byte
 *   aligned -- the alignment is examined before anything is launched and a buffer that misses it takes the generic kernels (the
 *   self-attention route of _bwd_h16 also wants loc / attn / grad_value on 16 bytes, as its output-tiled kernels do; otherwise the row
 *   kernel with the atomic scatter serves the call).  The fast forward and gather use 8 channels (16 bytes) per lane, or 4 where the
 *   per-row sample records of 8 would not fit the LDS; results do not depend on it beyond fp32 summation order.
 *   _bwd_h16 is the WHOLE backward for any shape.  shapes_host (may be NULL) and sel_state (may be NULL) as for ocpg_msda_bwd_f32 /
 *   ocpg_msda_bwd_value_sel_f32: with a host copy of the shapes, Lq == S and D in {16, 32} grad_value comes from the column-scatter /
 *   output-tiled kernels (which read grad_out in 16 bits) under the call site's path selection, grad_loc / grad_attn from the gather
 *   row kernel.  Forced paths: OCPG_MSDA_TILE / OCPG_MSDA_COL as documented above; the single-level column scatter that
 *   OCPG_MSDA_COL_LP < 4 forces reads fp32 only, so with it forced the whole 16-bit backward takes the generic kernel.
 *   shapes_host of _fwd_h16 is accepted for symmetry and not read.
 *   The fused front end has a 16-bit form of its own: ocpg_msda_fused_fwd_h16 / ocpg_msda_fused_bwd_qproj_h16 below. */
int ocpg_msda_fwd_h16(const void* value, const int64_t* shapes, const int64_t* level_start,
                      const float* loc, const float* attn,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      void* out, const int64_t* shapes_host, int dtype, void* stream);
int ocpg_msda_bwd_h16(const void* value, const int64_t* shapes, const int64_t* level_start,
                      const float* loc, const float* attn, const void* grad_out,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      float* grad_value, float* grad_loc, float* grad_attn,
                      const int64_t* shapes_host, int* sel_state, int dtype, void* stream);
/* The two halves of _bwd_h16 for the self-attention shape on their own, as ocpg_msda_bwd_value_sel_f32 / ocpg_msda_bwd_locattn_f32 (a
 * caller that wants only some gradients, or the two kernels timed apart).  -2000: shape, alignment or forced path not served, nothing
 * launched -- call ocpg_msda_bwd_h16 then. */
int ocpg_msda_bwd_value_h16(const float* loc, const float* attn, const void* grad_out,
                            int N, int S, int M, int D, int L, int Lq, int P,
                            float* grad_value, const int64_t* shapes_host, int* sel_state, int dtype, void* stream);
int ocpg_msda_bwd_locattn_h16(const void* value, const int64_t* shapes, const int64_t* level_start,
                              const float* loc, const float* attn, const void* grad_out,
                              int N, int S, int M, int D, int L, int Lq, int P,
                              float* grad_loc, float* grad_attn, int dtype, void* stream);
/* FUSED FRONT END with 16-bit storage: ocpg_msda_fused_fwd_f32 / ocpg_msda_fused_bwd_qproj_f32 (above) for a 16-bit value / out / grad_out.
 *   qproj, ref, loc_out, attn_out, loc, attn, grad_qproj: float32, laid out as for the _f32 symbols; value, out, grad_out: 16-bit
 *   elements of `dtype` (1 = bfloat16, 2 = float16; any other value returns an invalid-argument status and launches nothing).
 *   _fwd:       softmax over the 16 logits and `reference + offset` in fp32 in the row's sample set-up, loc_out / attn_out written in
 *               fp32, then the sampling of ocpg_msda_fwd_h16 (fp32 accumulation, `out` rounded to nearest-even once at its store).
 *   _bwd_qproj: the gather of ocpg_msda_bwd_locattn_h16 with the softmax backward in its epilogue; writes grad_qproj and nothing else
 *               (no atomics: bit-reproducible).  grad_value keeps coming from ocpg_msda_bwd_value_h16 with the call site's sel_state.
 *   Lane mapping as for the un-fused 16-bit kernels: 8 channels per lane by default, OCPG_MSDA_H16_LANES=4 forces 4.
 *   -2000 (nothing launched, every pointer examined first): D != 32, L*P != 16, value / out / grad_out off a 16-byte boundary, or
 *   qproj / ref / loc_out / grad_qproj off an 8-byte boundary.  The caller keeps ocpg_msda_fwd_h16 / ocpg_msda_bwd_h16 then. */
int ocpg_msda_fused_fwd_h16(const void* value, const int64_t* shapes, const int64_t* level_start,
                            const float* qproj, const float* ref,
                            int N, int S, int M, int D, int L, int Lq, int P,
                            void* out, float* loc_out, float* attn_out, int dtype, void* stream);
int ocpg_msda_fused_bwd_qproj_h16(const void* value, const int64_t* shapes, const int64_t* level_start,
                                  const float* loc, const float* attn, const void* grad_out,
                                  int N, int S, int M, int D, int L, int Lq, int P,
                                  float* grad_qproj, int dtype, void* stream);

/* Fused frozen-BatchNorm affine (+ residual) (+ ReLU) over a feature map -- replaces the per-BN elementwise chain of
 * FrozenBatchNorm2d.forward (models/backbone.py:46-56: x*scale + bias with scale = w*rsqrt(var+1e-5)) followed by
 * torchvision Bottleneck's "out += identity" / ReLU.  scale/shift are the per-channel fp32 vectors [C].
 *   y[o,c,i] = act(x[o,c,i] * scale[c] + shift[c] (+ skip[o,c,i])),  element (o,c,i) at ((o*C + c)*inner + i)
 *   NHWC / channels_last: n_outer = N*H*W, inner = 1;   NCHW: n_outer = N, inner = H*W.
 * dtype: 0 = float32, 1 = bfloat16, 2 = float16 (storage; arithmetic is fp32; narrowing rounds to nearest even, NaN / inf pass through and
 * an fp16 overflow becomes inf as in ATen: no saturation); anything else: -1010.  skip may be NULL.  y may alias x.
 * Backward needs only the saved OUTPUT y: g = relu ? (y > 0 ? gy : 0) : gy; gx = g*scale[c]; gskip = g.
 * gx or gskip may be NULL (not wanted); gskip may alias gy. */
int ocpg_bn_act_fwd(const void* x, const float* scale, const float* shift, const void* skip, void* y,
                    long long n_outer, int C, long long inner, int relu, int dtype, void* stream);
int ocpg_bn_act_bwd(const void* gy, const void* y, const float* scale, void* gx, void* gskip,
                    long long n_outer, int C, long long inner, int relu, int dtype, void* stream);

/* Input gradient of a 1x1 convolution (channels-last bf16 or fp16) with the frozen-BN + ReLU backward of the layer in front in its epilogue
 * (csrc/gemm_dgrad_bn.hip; MFMA, fp32 accumulation): replaces ocpg_gemm (input gradient) + ocpg_bn_act_bwd of the layer in front.
 *   v[m,n] = sum_k a[m,k] w[k,n]         a [M,K] (the gradient after this convolution's BN backward), w [K = Cout][N = Cin] as it lies
 *   v += c[m,n]                          c may be NULL; the block's parked identity-skip gradient
 *   v  = mask[m,n] > 0 ? v : 0           mask may be NULL; the convolution's own input = that layer's post-ReLU output
 *   out_skip[m,n] = bf16(v)              out_skip may be NULL, and may be c itself (in place)
 *   out[m,n] = bf16(v * scale[n])        scale fp32 [N] or NULL (= 1)
 * tile: 0 = 128 x 128, 1 = 64 x 128, 2 = 64 x 64 workgroup tiles; ocpg_gemm_dgrad_bn_tile returns the measured-best one (64 x 64) or -1
 * (the shape is not served).  Deterministic; every tile gives the same bits.
 * Declined (the caller keeps its GEMM + ocpg_bn_act_bwd): -2000 shape (N % tile width, K % 128), -2001 a pointer not 16-byte aligned,
 * -2002 dtype other than 1 (bf16) or 2 (fp16: its own instantiations, MFMA 32x32x16 f16; `bf16(...)` above then reads fp16(...)). */
int ocpg_gemm_dgrad_bn_tile(long long M, int N, int K);
int ocpg_gemm_dgrad_bn(const void* a, const void* w, const void* c, const void* mask, const float* scale, void* out, void* out_skip,
                       long long M, int N, int K, int dtype, int tile, void* stream);

/* The encoder FFN's bias + ReLU + dropout passes as epilogues of the same tile code (bf16 only; tiles as above, every tile the same bits).
 * Backward, linear2's input gradient with ocpg_bias_relu_dropout_bwd in its epilogue:
 *   v[m,n] = sum_k a[m,k] w[k,n]                 a [M,K] the gradient at linear2's output, w = linear2.weight [K][N] as it lies
 *   g      = mask[m,n] > 0 ? v * scale : 0       mask = the saved hidden map h (zero where ReLU or dropout zeroed it), scale = 1/(1-p)
 *   out[m,n] = bf16(g)
 *   colsum_part[t][n] = sum of g (fp32, before narrowing) over the valid rows of row tile t, t < ceil(M / tile rows (128, 64, 64)):
 *                       plain stores, every element written exactly once, fixed order, no atomics (the caller sums the tiles: the bias gradient)
 * Forward, linear1 with ocpg_bias_relu_dropout_fwd in its epilogue:
 *   h[m,n] = bf16(max(sum_k x[m,k] w[n,k] + bias[n], 0) * keep)      w = linear1.weight [N][K] as it lies; keep = 0 or 1/(1-p), drawn as
 *   ocpg_bias_relu_dropout_fwd draws it (counter (m N + n) / 4, offset + *rng_base): the same (seed, offset) gives the same mask; p = 0 draws nothing.
 *   round_gemm != 0: h[m,n] = bf16(max(bf16(sum) + bias[n], 0) * keep), the arithmetic of the pair (a bf16 GEMM result, then the pass): the same h
 *   wherever both GEMMs' fp32 sums round to the same bf16 value.  0 is one rounding closer to the exact result, but a pre-activation within a
 *   bf16 spacing of zero can then fall on the other side of the ReLU than the pair puts it.
 * Neither call allocates.  Declined exactly as ocpg_gemm_dgrad_bn declines (-2000 shape, -2001 alignment, -2002 dtype other than 1). */
int ocpg_gemm_dgrad_mask(const void* a, const void* w, const void* mask, float scale, void* out, float* colsum_part, long long M, int N,
                         int K, int dtype, int tile, void* stream);
int ocpg_gemm_bias_relu_dropout_fwd(const void* x, const void* w, const void* bias, float p, unsigned long long seed,
                                    unsigned long long offset, const unsigned long long* rng_base, void* h, long long M, int N, int K,
                                    int dtype, int tile, int round_gemm, void* stream);

/* Fused 3-D (shifted-)window attention of Video-Swin -- replaces WindowAttention3D.forward's score / bias / mask /
 * softmax / PV chain (models/video_swin_transformer.py:138-169) and the shift-mask tensor of compute_mask (:316-329).
 *   qkv    [BW, N, 3, H, head_dim]   output of the qkv Linear (BW = batch * windows), head_dim must be 32
 *   bias   [H, N, N]  relative-position bias (query i, key j);  biasT [H, N, N] the same transposed (key j, query i)
 *   region [NW, N] int32 cyclic-shift region id of every window slot, or NULL (no shift); window = bw % NW;
 *          a (query, key) pair in different regions gets -100 added, exactly like the reference's mask
 *   out    [BW, N, H*head_dim];  lse [BW, H, N] fp32 log-sum-exp of every row (saved for the backward)
 * dtype: 0 float32, 1 bfloat16, 2 float16 (storage of qkv/out/dout/dqkv; arithmetic and bias/lse are fp32).
 * Backward: dqkv [BW, N, 3, H, head_dim] fully overwritten; Dbuf [BW, H, N] fp32 scratch;
 * dbiasT [H, N, N] fp32 is ACCUMULATED into (caller zeroes it; may be NULL when the bias needs no gradient). */
int ocpg_win_attn_fwd(const void* qkv, const float* biasT, const int* region, float scale, int BW, int NW, int N, int H,
                      int head_dim, void* out, float* lse, int dtype, void* stream);
int ocpg_win_attn_bwd(const void* qkv, const float* bias, const float* biasT, const int* region, float scale, int BW, int NW,
                      int N, int H, int head_dim, const void* out, const void* dout, const float* lse, void* dqkv, float* Dbuf,
                      float* dbiasT, int dtype, void* stream);

/* Matrix-core backward for bf16 / fp16 storage (csrc/win_attn_mfma.hip; the forward switches by itself): as ocpg_win_attn_bwd, but
 * the bias gradient leaves as dS [BW, H, N, N] (storage dtype, (key, query) order, fully written; NULL: not needed) for the caller to
 * sum over BW -- 2 x 232 MB of streaming traffic at Swin-T stage 1 instead of 464 MB of float atomics.  -2000: shape not served. */
int ocpg_win_attn_bwd_mfma(const void* qkv, const float* bias, const float* biasT, const int* region, float scale, int BW, int NW, int N,
                           int H, int head_dim, const void* out, const void* dout, const float* lse, void* dqkv, float* Dbuf, void* dS,
                           int dtype, void* stream);

/* Opt-in variant of ocpg_win_attn_bwd_mfma that returns the gradient of the relative-position TABLE [T, H] and writes no dS: the bias
 * is table[idx[q, key]] with idx[q, key] = tok_code[q] - tok_code[key] + code_off (tok_code [N] int32; the caller guarantees [0, T)).  Each
 * (window, head) sums its dS (fp32, un-rounded) into T floats of LDS and stores them to partials [BW, H, T] (fp32 workspace); a second
 * kernel sums over the windows in a fixed order into dtable [T, H].  Both are fully written, rows no pair addresses as exact zeros:
 * nothing to zero beforehand, no global atomics.  ocpg_win_attn_dtable_supported: 1 when N / head_dim / dtype / T are served (the LDS
 * holds K, V, the N codes and the T floats) and OCPG_WIN_ATTN_MFMA is not 0, else 0; launches nothing.  The backward returns -2000 in
 * exactly the cases where that answer is 0, before anything is launched. */
int ocpg_win_attn_dtable_supported(int N, int head_dim, int dtype, int T);
int ocpg_win_attn_bwd_mfma_dtable(const void* qkv, const float* bias, const float* biasT, const int* region, float scale, int BW, int NW,
                                  int N, int H, int head_dim, const void* out, const void* dout, const float* lse, void* dqkv, float* Dbuf,
                                  const int* tok_code, int code_off, int T, float* partials, float* dtable, int dtype, void* stream);

/* Dynamic (per-query) mask head, forward -- replaces OCPG.dynamic_mask_with_coords + mask_heads_forward
 * (models/ocpg.py:475-549) for the reference's fixed head shape (2 layers, 16 channels, relative coordinates on).
 * Q counts the parameter sets per frame: the reference calls the head once per decoder layer on the SAME mask features
 * (ocpg.py:339-349); passing Q = layers x queries does all of them in one launch.
 *   feats  [BT, C, H, W] fp32 mask features;  params [BT*Q, (C+2)*16 + 16*16 + 16 + 16] controller outputs in the
 *   reference's order (parse_dynamic_params, ocpg.py:552-569: W0 [16,(C+2)] incl. the x,y coordinate columns, W1 [16,16],
 *   b0, b1);  refpix [BT*Q, 2] reference point in INPUT pixels (ref_xy * (img_w, img_h));  stride = mask_feat_stride (8)
 *   out    [BT*Q, 16, H, W];  pre1 [BT*Q, 16, H, W] = layer-1 pre-activation (kept for the backward; may be NULL). */
int ocpg_dynmask_fwd_f32(const float* feats, const float* params, const float* refpix, int BT, int Q, int C, int H, int W,
                         int stride, float* out, float* pre1, void* stream);

/* Backward of the dynamic mask head (autograd of models/ocpg.py:505-549 in the reference), all decoder layers per launch.
 * _pre: dout, pre1 [BT*Q,16,H,W] -> dpre [BT*Q,16,H,W] = (W1^T dout) * (pre1 > 0); part [BT*Q, ceil(HW/256), 320] per-strip
 *       partial sums (dW1 16x16 | db0 | db1 | sum dpre*x | sum dpre*y); w0d [BT*Q,16,C] = the feature columns of W0, dense.
 *       The two large contractions dW0 = dpre . feats^T and dfeat = W0^T . dpre are plain GEMMs on these buffers (ocpg_gemm).
 * _fin: part + dw0 [BT*Q,16,C] (the dW0 GEMM's result) -> dparams [BT*Q, (C+2)*16+16*16+32] fully written in the reference's
 *       parameter order (parse_dynamic_params, ocpg.py:552-569) and dref [BT*Q,2] (may be NULL). */
int ocpg_dynmask_bwd_pre_f32(const float* dout, const float* pre1, const float* params, int BT, int Q, int C, int H, int W,
                             int stride, float* dpre, float* part, float* w0d, void* stream);
int ocpg_dynmask_bwd_fin_f32(const float* part, const float* params, const float* refpix, const float* dw0, int BT, int Q, int C,
                             int H, int W, float* dparams, float* dref, void* stream);

/* 3x3 convolution of channels-last maps as one dense GEMM -- replaces the conv kernels behind nn.Conv2d(k=3) in the ResNet
 * body (torchvision Bottleneck.conv2 via models/backbone.py:86-117) and the neck (models/ocpg.py:118-126); the GEMM itself
 * is hipBLASLt's.  Geometry: kernel 3x3, padding == dil, stride in {1,2}; Ho = (H-1)/stride + 1, Wo likewise.
 *   im2col: x [N,H,W,C] -> cols [N*Ho*Wo, 9*C], column order (ky, kx, c) = the physical order of a channels-last weight
 *   col2im: dcols [N*Ho*Wo, 9*C] -> dx [N,H,W,C] (the adjoint: every dx element fully written, fp32 accumulation)
 * dtype: 0 fp32, 1 bf16, 2 fp16; C * sizeof(elem) must be a multiple of 16. */
int ocpg_im2col3x3_nhwc(const void* x, int N, int H, int W, int C, int stride, int dil, void* cols, int dtype, void* stream);
int ocpg_col2im3x3_nhwc(const void* dcols, int N, int H, int W, int C, int stride, int dil, void* dx, int dtype, void* stream);

/* 3x3 convolution (padding 1, stride 1 | 2) of channels-last bf16 maps as an implicit GEMM on the matrix cores
 * (csrc/conv3x3_mfma.hip: MFMA 32x32x16 bf16, fp32 accumulation, no im2col buffer) -- replaces the MIOpen kernels behind
 * torchvision Bottleneck.conv2 (models/backbone.py:86-117) and, in its epilogue, FrozenBatchNorm2d's affine + ReLU
 * (models/backbone.py:46-56).
 *   fwd:   x [N,H,W,Cin], w [Cout,3,3,Cin] (a channels-last weight as it lies in memory) -> y [N,Ho,Wo,Cout] =
 *          act(conv(x, w) * scale[co] + bias[co]); scale / bias fp32 or NULL; Cin % 32 == 0.
 *   dgrad: dy [N,Ho,Wo,Cout], wT [Cin,3,3,Cout] (channel axes swapped, taps NOT flipped) -> dx [N,H,W,Cin] fully written;
 *          Cout % 32 == 0.
 * -2000: geometry not served (the caller keeps its other path).  The weight gradient is a GEMM over the im2col matrix
 * (ocpg_im2col3x3_nhwc + ocpg_gemm). */
int ocpg_conv3x3_mfma_fwd(const void* x, const void* w, const float* scale, const float* bias, int relu, int N, int H, int W,
                          int Cin, int Cout, int stride, void* y, void* stream);
/* the same, and the patch (im2col) matrix of x written on the way: cols [N*Ho*Wo, 9*Cin] bf16 in (ky, kx, ci) column order (what
 * ocpg_im2col3x3_nhwc produces), or NULL -- the weight gradient of the convolution contracts the output gradient with it. */
int ocpg_conv3x3_mfma_fwd_cols(const void* x, const void* w, const float* scale, const float* bias, int relu, int N, int H, int W, int Cin,
                               int Cout, int stride, void* y, void* cols, void* stream);
int ocpg_conv3x3_mfma_dgrad(const void* dy, const void* wT, int N, int H, int W, int Cin, int Cout, int stride, void* dx,
                            void* stream);
/* ocpg_conv3x3_mfma_dgrad that ALSO applies the frozen-BN + ReLU backward of the layer in front (round 4; FrozenBatchNorm2d backbone.py:46-56
 * + ReLU of torchvision's Bottleneck between conv1 and conv2): dx[n,h,w,ci] = conv_transpose(dy)[n,h,w,ci] * scale[ci] where
 * mask_y[n,h,w,ci] > 0, else 0.  mask_y = that layer's post-ReLU output (the convolution's own input), bf16, laid out like dx; scale fp32
 * [Cin] or NULL (= 1).  Saves one ocpg_bn_act_bwd pass per bottleneck. */
int ocpg_conv3x3_mfma_dgrad_masked(const void* dy, const void* wT, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                   int Cout, int stride, void* dx, void* stream);
/* The same from the convolution's OWN weight w [Cout, 3, 3, Cin] (round 4: no transposed copy per step; the kernel reads its weight
 * fragments with transposing LDS loads).  mask_y / scale as above (NULL: plain input gradient).  Cin % 8 != 0: -2000. */
int ocpg_conv3x3_mfma_dgrad_w(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin, int Cout,
                              int stride, void* dx, void* stream);
/* Weight gradient of the same convolution straight from the two channels-last maps (csrc/conv3x3_wgrad.hip; round 4: replaces
 * ocpg_im2col3x3_nhwc + a row-split ocpg_gemm): gz [N,Ho,Wo,Cout] bf16 (the gradient after the BN / ReLU backward), x [N,H,W,Cin] bf16 ->
 * part [S][Cout][3][3][Cin] bf16, S = ocpg_conv3x3_mfma_wgrad_splits(...) partial sums over ranges of output rows (the caller adds them:
 * gw = sum_z part[z]).  Cin % 8 or Cout % 8 != 0: -2000. */
/* The same forward / input gradient with the K chain split over the grid for launches of few tiles and long K (round 4: ResNet layer3 /
 * layer4 at 1-2 clips per step): `splits` = ocpg_conv3x3_mfma_body_splits(rows, GEMM columns, K channels) (1 = use the un-split entry);
 * part: fp32 scratch [splits][rows][columns]; the summing pass applies the epilogue (BN affine + ReLU; scale + mask of the layer in front). */
int ocpg_conv3x3_mfma_body_splits(long long M, int ncols, int kchannels);
int ocpg_conv3x3_mfma_fwd_bn_splitk(const void* x, const void* w, const float* scale, const float* shift, int relu, int N, int H, int W, int Cin,
                                    int Cout, int stride, int splits, float* part, void* y, void* stream);
int ocpg_conv3x3_mfma_dgrad_w_splitk(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin,
                                     int Cout, int stride, int splits, float* part, void* dx, void* stream);
int ocpg_conv3x3_mfma_wgrad_splits(int N, int H, int W, int Cin, int Cout, int stride);
int ocpg_conv3x3_mfma_wgrad(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, void* stream);
/* The three entry points of the shipped step with the 16-bit STORAGE TYPE as an argument (the reference's --amp mode is fp16:
 * engine.py amp.autocast + GradScaler): dtype 1 = bfloat16, 2 = float16 (the numbering of ocpg_bn_act_* and of the MSDeformAttn _h16 entry
 * points); any other value returns -1010 before anything is launched.  Arguments, geometry limits and return codes are those of the
 * un-suffixed twin, every tensor (x, w, y, cols / dy, mask_y, dx / gz, part) in that one type; scale / bias stay fp32 and the accumulation
 * fp32.  With dtype 1 they launch the very kernels the un-suffixed symbols launch (which forward here); with dtype 2 the fp16 instantiations
 * (MFMA 32x32x16 f16).  ocpg_conv3x3_mfma_wgrad_splits serves both.  The neck's split-K forward has its fp16 form below
 * (ocpg_conv3x3_mfma_fwd_splitk_h16); the body split-K pair (ocpg_conv3x3_mfma_fwd_bn_splitk, ocpg_conv3x3_mfma_dgrad_w_splitk),
 * ocpg_conv3x3_mfma_dgrad(_masked) and the halo variant have no fp16 form. */
int ocpg_conv3x3_mfma_fwd_cols_h16(const void* x, const void* w, const float* scale, const float* bias, int relu, int N, int H, int W, int Cin,
                                   int Cout, int stride, void* y, void* cols, int dtype, void* stream);
int ocpg_conv3x3_mfma_dgrad_w_h16(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin, int Cout,
                                  int stride, void* dx, int dtype, void* stream);
int ocpg_conv3x3_mfma_wgrad_h16(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, int dtype,
                                void* stream);
/* ocpg_conv3x3_mfma_wgrad(_h16) by the ring kernel (csrc/conv3x3_wgrad_ring_kernel.h): input rows roll through an LDS ring (a step fetches
 * only the rows the ring does not hold yet), one barrier per step, 8 waves with the nine taps split 5 + 4.  Same arguments, checks in the
 * same order, return codes, split (ocpg_conv3x3_mfma_wgrad_splits) and `part` layout as the twin, and every element of `part` bit-identical
 * to the twin's (each accumulator sees the same 16-pixel k steps in the same order).  Served: maps of one segment per output row
 * (Wo <= 64 under stride 1, Wo <= 32 under stride 2); a wider map returns -2000 before any launch, `part` untouched: call the twin. */
int ocpg_conv3x3_mfma_wgrad_ring(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, void* stream);
int ocpg_conv3x3_mfma_wgrad_ring_h16(const void* gz, const void* x, int N, int H, int W, int Cin, int Cout, int stride, void* part, int dtype,
                                     void* stream);
/* ocpg_conv3x3_mfma_dgrad_w(_h16) for stride 2 in parity-class tiles: a 64-row tile holds input pixels of one class (y & 1, x & 1) and walks
 * only the taps that reach it (4 for odd/odd, 2 for the mixed classes, 1 for even/even: 9 taps per 4 pixels, where the nine-tap symbols
 * walk 36 and multiply zero rows for 27 of them).  Same arguments, checks and return codes as the nine-tap twin; stride != 2 returns -2000.
 * dx is fully written and, for finite operands, bit-identical to the nine-tap symbol's (the same non-zero products in the same order). */
int ocpg_conv3x3_mfma_dgrad_w_s2(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin, int Cout,
                                 int stride, void* dx, void* stream);
int ocpg_conv3x3_mfma_dgrad_w_s2_h16(const void* dy, const void* w, const void* mask_y, const float* scale, int N, int H, int W, int Cin, int Cout,
                                     int stride, void* dx, int dtype, void* stream);

/* Split-K form of ocpg_conv3x3_mfma_fwd for convolutions with FEW output pixels and a LONG reduction (round 4): the neck's extra level
 * input_proj[3] = nn.Conv2d(2048, 256, 3, stride=2, padding=1) (models/ocpg.py:119-123; 600 output pixels at config #2, K = 18 432) --
 * MIOpen's split-K kernel until round 3.  blockIdx.z takes a contiguous range of 64-channel chunks; the tiles leave as fp32 partial
 * sums part[splits][N*Ho*Wo][Cout] (caller-provided scratch, fully written) and a second kernel adds them and the bias into
 * y [N,Ho,Wo,Cout] (out_dt 0 fp32 / 1 bf16).  ocpg_conv3x3_mfma_splits: the number of ranges to use for a shape (1 = the plain kernel
 * fills the chip: call ocpg_conv3x3_mfma_fwd).  cols (may be NULL): the patch matrix, as ocpg_conv3x3_mfma_fwd_cols writes it.  The input
 * gradient is ocpg_conv3x3_mfma_dgrad (its GEMM has N*H*W rows: no split needed).
 * _h16: the same with the 16-bit storage type of x / w / cols as an argument, by the convention of the _h16 symbols above: dtype 1 =
 * bfloat16 (the very launches of the un-suffixed symbol, which forwards here), 2 = float16 (the fp16 instantiation of the kernel); any
 * other value returns -1010 before any other check.  out_dt is 0 (fp32) or equal to dtype; anything else returns -2000.  Every other check,
 * limit and return code is the un-suffixed symbol's.  In fp16 the input gradient is ocpg_conv3x3_mfma_dgrad_w_h16 on the convolution's
 * own weight with a NULL mask and a NULL scale (ocpg_conv3x3_mfma_dgrad is bf16-only). */
int ocpg_conv3x3_mfma_splits(int N, int H, int W, int Cin, int Cout, int stride);
int ocpg_conv3x3_mfma_fwd_splitk(const void* x, const void* w, const float* bias, int N, int H, int W, int Cin, int Cout, int stride,
                                 int splits, float* part, void* y, int out_dt, void* cols, void* stream);
int ocpg_conv3x3_mfma_fwd_splitk_h16(const void* x, const void* w, const float* bias, int N, int H, int W, int Cin, int Cout, int stride,
                                     int splits, float* part, void* y, int out_dt, void* cols, int dtype, void* stream);

/* Dense GEMM with a per-shape plan cache over hipBLASLt -- replaces the at::mm / at::addmm / at::bmm calls behind
 * nn.Linear and the 1x1 nn.Conv2d layers on the path (models/deformable_transformer.py:236-257,313-327 FFNs,
 * models/ops/modules/ms_deform_attn.py:63-66 projections, torchvision Bottleneck.conv1/conv3 via models/backbone.py) and
 * their gradients; same hipBLASLt kernels, ~1/3 of the host cost per call (the step is launch-bound).
 * Row-major:  C[M,N] = alpha * op(A) op(B) + beta * C (+ bias[N]);  op(A) = A [M,K] (lda) or A^T with A stored [K,M];
 * op(B) = B [K,N] (ldb) or B^T with B stored [N,K].  batch > 1: strided batches (element strides).  dtype / out_dtype:
 * 0 fp32, 1 bf16, 2 fp16 (fp32 accumulation).  State (handle, plans) is per device, the 64-MB workspace per (device, stream). */
int ocpg_gemm(const void* A, const void* B, void* C, const void* bias, int dtype, int out_dtype, int transA, int transB,
              long long M, long long N, long long K, long long lda, long long ldb, long long ldc, long long batch,
              long long strideA, long long strideB, long long strideC, float alpha, float beta, void* stream);
long long ocpg_gemm_plans(void);      /* number of cached plans (diagnostics) */
/* Plan selection: the first call of a plan that can be repeated without changing its result (beta == 0; the BN form with skip != D)
 * times hipBLASLt's ranked candidates on the caller's operands (eager calls only, never inside a stream capture) and keeps the
 * fastest one whose result agrees with the heuristic's single choice (what at::mm runs) to the rounding of the output type (8e-3 /
 * 1e-3 of max |C| for bf16 / fp16 outputs).  bf16 / fp16 plans only: fp32 plans always keep the heuristic's choice (its ranked fp32
 * list holds kernels that are 2e-3 off).  OCPG_GEMM_TUNE=0 keeps the heuristic's choice everywhere;
 * OCPG_GEMM_TUNE_FP32=1 (experiment, off by default) also times fp32 plans, validated to 1e-5 of max |C|.  ocpg_gemm_tuned returns the number of plans timed on the current device and, in *changed (may be NULL),
 * how many of them left the first choice; ocpg_gemm_tune_rejected the number of candidates dropped for a differing result. */
long long ocpg_gemm_tuned(long long* changed);
long long ocpg_gemm_tune_rejected(void);
/* Rank-consistent plan choices for data-parallel training (the role of the reference's main.py:62 DistributedDataParallel ranks running
 * one cuBLAS build: every rank must run the same GEMM kernels, or the slowest rank's choice sets the step).  The candidate timing above is
 * a per-process measurement, so under N > 1 ranks ONE rank times (ocpg_gemm_set_tuning(0) on the others before their first GEMM),
 * exports its choices as [key hash, candidate index] pairs, the caller broadcasts them, and every other rank imports them: they apply to
 * the plans that already exist and to those built later (the heuristic's ranked candidate list is identical on identical hardware).
 * set_tuning: 1 / 0 = candidate timing on / off in this process, -1 = OCPG_GEMM_TUNE decides.  export: returns the number of pairs
 * (buf may be NULL to ask for the count); import: 0 on success. */
void ocpg_gemm_set_tuning(int on);
long long ocpg_gemm_export_picks(long long* buf, long long cap_pairs);
int ocpg_gemm_import_picks(const long long* buf, long long n_pairs);
/* D[M,N] = act(scale[n] * (A W^T)[m,n] + shift[n] (+ skip[m,n])): the 1x1 conv + FrozenBatchNorm2d affine (+ identity) (+ ReLU) of a
 * Bottleneck (models/backbone.py:46-56 + torchvision's block) inside the GEMM epilogue (per-channel alpha vector, fp32 bias, ReLU,
 * beta = 1 on the skip operand).  A [M,K], W [N,K], skip / D [M,N] dense row-major, dtype 0/1/2; scale, shift fp32 [N].
 * Returns -1105 when hipBLASLt offers no kernel for the combination (fall back to ocpg_gemm + ocpg_bn_act_fwd). */
int ocpg_gemm_bn_act(const void* A, const void* W, void* D, const float* scale, const float* shift, const void* skip, int relu, int dtype,
                     long long M, long long N, long long K, void* stream);

/* Mask-criterion losses, all decoder layers per call (fp32; replace the elementwise/reduction chains of
 * models/segmentation.py:203-211,253-315 as called from models/criterion.py:141-178).
 *
 * Level-set loss: x [Lr,N,h,w] logits, feats [N,CF,h,w] (first C channels used, C <= 16), box [N,h,w] in {0,1}.
 *   fwd: sums [Lr,N,ceil(h*w/1024),7+2C] scratch (per-workgroup partials), coef [Lr,N,8+2C] kept for the backward; loss [Lr], the
 *        N per-frame terms added in ascending n (no atomics: the same bits on every call).
 *   bwd: gloss [Lr] upstream gradient -> gx [Lr,N,h,w], gfeat [N,CF,h,w] (may be NULL), both fully written. */
int ocpg_levelset_fwd_f32(const float* x, const float* feats, const float* box, int Lr, int N, int C, int CF, int h, int w, float* sums,
                          float* coef, float* loss, void* stream);
int ocpg_levelset_bwd_f32(const float* x, const float* feats, const float* box, const float* coef, const float* gloss, int Lr, int N,
                          int C, int CF, int h, int w, float* gx, float* gfeat, void* stream);
/* Box-projection loss with mean term: x [Lr,B,T,H,W] logits; targets tcmax/tcmean [B,T,W] (region.amax / weak.mean over H),
 * trmax/trmean [B,T,H] (over W).  fwd: colstat [Lr*B*T,3,W], rowstat [Lr*B*T,3,H], IU [Lr,B,4,2] scratch kept for the
 * backward; loss [Lr].  bwd: Gc [Lr*B*T,2,W], Gr [Lr*B*T,2,H] scratch; gx [Lr,B,T,H,W] fully written. */
int ocpg_proj_fwd_f32(const float* x, const float* tcmax, const float* trmax, const float* tcmean, const float* trmean, int Lr, int B,
                      int T, int H, int W, float* colstat, float* rowstat, float* IU, float* loss, void* stream);
int ocpg_proj_bwd_f32(const float* x, const float* tcmax, const float* trmax, const float* tcmean, const float* trmean,
                      const float* colstat, const float* rowstat, const float* IU, const float* gloss, int Lr, int B, int T, int H, int W,
                      float* Gc, float* Gr, float* gx, void* stream);

/* Matching cost [Lr,B,Q] of every query against the clip's single target -- replaces the cost construction of
 * HungarianMatcher.forward (models/matcher.py:74-160) for all decoder layers: wc * focal-class (mean over valid frames) +
 * wb * L1 + wg * (-GIoU) (means over frames) + wm * sigmoid-focal + wd * (-dice) (over the clip's pixels).
 * logits [Lr,B,T,Q,K], boxes [Lr,B,T,Q,4] cxcywh, contiguous; masks: logits with element strides (sl,sb,st,sq) for
 * (layer, clip, frame, query) and a contiguous [h,w] tail; gt [B,T,h,w]; tboxes [B,T,4]; valid [B,T] (float);
 * labels [B,T] int64 or NULL (class 0).  sums [Lr,B,Q,4] scratch.  bad: optional int32 counter, +1 per (layer,clip,query)
 * with a malformed box. */
int ocpg_matcher_cost_f32(const float* logits, const float* boxes, const float* masks, long long sl, long long sb, long long st,
                          long long sq, const float* gt, const float* tboxes, const float* valid, const long long* labels, int Lr,
                          int B, int T, int Q, int K, int h, int w, float wc, float wb, float wg, float wm, float wd, float* sums,
                          float* cost, int* bad, void* stream);

/* Transformer-layer glue (models/deformable_transformer.py:236-257,313-336), one HBM pass each way:
 *   y = LayerNorm(res + dropout(x)):  x [R,C] (x_dtype 0 fp32 / 1 bf16), res / y fp32, C % 4 == 0, C <= 2048; mean, rstd [R]
 *     are kept for the backward, which recomputes the dropout mask from (seed, offset) (Philox-4x32-10, counter = element/4);
 *     rng_base: NULL, or a DEVICE pointer to one 64-bit word that the kernel adds to `offset` when it runs -- a call captured
 *     into a HIP graph bakes `offset` into the node, so the caller keeps the per-step base in device memory and advances it
 *     between replays (every replay then draws fresh masks, as models/deformable_transformer.py:236-257 does every step);
 *     bwd: gx (x's dtype, may be NULL), gres (may be NULL) fully written; dgb_part [slots, 2, C] partial (dgamma, dbeta) sums,
 *     fully written, slots = ocpg_dropout_add_ln_bwd_slots(R); the caller sums over the slots.
 *     The _ex symbols are the same kernels with more ports (with every extra absent and g0 fp32: the un-suffixed kernels, bit for bit).
 *     fwd_ex: addend + y_add (both or neither, fp32 [R,C]): y_add = y + addend, one fp32 add of the value stored as y; y_lp (may be
 *     NULL): y rounded to nearest even to lp_dtype (1 bf16 / 2 fp16).  bwd_ex: gy = (g0 + g1) + g2 in that order, each addend [R,C] of
 *     its own dtype (0 / 1 / 2) widened to fp32 first, g1 / g2 may be NULL; gxsum_part (may be NULL) [slots, C]: per slot, the column
 *     sums of gx as stored (rounded to x's dtype, then widened) -- the bias gradient of the Linear that produced x, summed over the
 *     slots by the caller.
 *   h = dropout(relu(a + bias)):  a, bias, h share dtype (0 fp32 / 1 bf16), h may alias a; bwd from h only:
 *     ga = gh / (1-p) where h > 0; dbias_part [slots, C] fp32 partial column sums, fully written, slots =
 *     ocpg_bias_relu_dropout_bwd_slots(R, C, dtype); the caller sums over the slots. */
int ocpg_dropout_add_ln_fwd(const void* x, const float* res, const float* gamma, const float* beta, long long R, int C, float eps, float p,
                            unsigned long long seed, unsigned long long offset, const unsigned long long* rng_base, int x_dtype, float* y,
                            float* mean, float* rstd, void* stream);
int ocpg_dropout_add_ln_bwd(const float* gy, const void* x, const float* res, const float* gamma, const float* mean, const float* rstd,
                            long long R, int C, float p, unsigned long long seed, unsigned long long offset, const unsigned long long* rng_base,
                            int x_dtype, void* gx, float* gres, float* dgb_part, void* stream);
long long ocpg_dropout_add_ln_bwd_slots(long long R);
int ocpg_dropout_add_ln_fwd_ex(const void* x, const float* res, const float* gamma, const float* beta, long long R, int C, float eps, float p,
                               unsigned long long seed, unsigned long long offset, const unsigned long long* rng_base, int x_dtype, float* y,
                               float* mean, float* rstd, const float* addend, float* y_add, void* y_lp, int lp_dtype, void* stream);
int ocpg_dropout_add_ln_bwd_ex(const void* g0, int g0_dtype, const void* g1, int g1_dtype, const void* g2, int g2_dtype, const void* x,
                               const float* res, const float* gamma, const float* mean, const float* rstd, long long R, int C, float p,
                               unsigned long long seed, unsigned long long offset, const unsigned long long* rng_base, int x_dtype, void* gx,
                               float* gres, float* dgb_part, float* gxsum_part, void* stream);
int ocpg_bias_relu_dropout_fwd(const void* a, const void* bias, long long R, int C, float p, unsigned long long seed,
                               unsigned long long offset, const unsigned long long* rng_base, int dtype, void* h, void* stream);
int ocpg_bias_relu_dropout_bwd(const void* gh, const void* h, long long R, int C, float p, int dtype, void* ga, float* dbias_part,
                               void* stream);
long long ocpg_bias_relu_dropout_bwd_slots(long long R, int C, int dtype);

/* Dtype cast of MANY dense tensors in one launch -- replaces the per-parameter autocast casts and the per-parameter
 * gradient casts of an AMP step (torch.cuda.amp as used by engine.py:49-62).  Device tables (int64): srcs / dsts = element
 * pointers, numels, chunk_prefix [n+1] = prefix sum of ceil(numel / 2048); total_chunks = chunk_prefix[n].
 * dtype codes: 0 fp32, 1 bf16, 2 fp16; supported pairs: fp32 <-> bf16, fp32 <-> fp16. */
int ocpg_multi_cast(const long long* srcs, const long long* dsts, const long long* numels, const long long* chunk_prefix, int n,
                    long long total_chunks, int src_dtype, int dst_dtype, void* stream);
/* The same with a reduction on the way: tensor t = sum of splits[t] slices of numels[t] elements, strides[t] elements apart (the
 * row-split weight-gradient partial products of the fused conv nodes: replaces one at::sum launch per layer, ~90 per step in the
 * ResNet body of models/backbone.py, plus the cast).  src_dtype 0 fp32 / 1 bf16 / 2 fp16 -> fp32; fp32 accumulation. */
int ocpg_multi_cast_sum(const long long* srcs, const long long* dsts, const long long* numels, const long long* chunk_prefix,
                        const long long* splits, const long long* strides, int n, long long total_chunks, int src_dtype, int dst_dtype,
                        void* stream);
/* Partial column sums of x [R, C] (dtype 0 fp32 / 1 bf16 / 2 fp16) -> part [ocpg_colsum_blocks(R), C] fp32, fully written: the
 * bias gradient `grad_output.sum(0)` of nn.Linear / a 1x1 nn.Conv2d over many rows (models/deformable_transformer.py:236-257 FFNs,
 * models/modules.py:12-16 LFM convolutions) as ONE launch; ocpg_multi_cast_sum finishes the sum over the blocks. */
long long ocpg_colsum_blocks(long long R);
int ocpg_colsum_partials(const void* x, long long R, int C, int dtype, float* part, void* stream);

/* Gradient clipping + AdamW over MANY fp32 tensors (device tables of pointers / element counts / 2048-element chunk prefixes, as
 * ocpg_multi_cast) -- replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step of engine.py:100-106 / main.py:76-99:
 *   ocpg_grad_norm_clip: partials [total_chunks] (scratch) -> norm_and_coef[0] = total 2-norm of all gradients,
 *                        norm_and_coef[1] = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0); two launches;
 *   ocpg_adamw_step:     p, exp_avg, exp_avg_sq updated in one launch; the gradient is multiplied by norm_and_coef[1] on the fly (NULL:
 *                        no clipping); lr / weight_decay: per-tensor fp32 device arrays (the optimizer's groups); step >= 1 is the
 *                        step count AFTER this update (bias corrections).  betas / eps are doubles: 1 - beta is formed in double, as
 *                        torch's Python scalars are (1.f - 0.999f is 4.7e-5 off 0.001).  Arithmetic = torch's single-tensor AdamW. */
int ocpg_grad_norm_clip(const long long* grads, const long long* numels, const long long* chunk_prefix, int n, long long total_chunks,
                        float max_norm, float* partials, float* norm_and_coef, void* stream);
int ocpg_adamw_step(const long long* params, const long long* grads, const long long* exp_avg, const long long* exp_avg_sq,
                    const long long* numels, const long long* chunk_prefix, const float* lr, const float* weight_decay, int n,
                    long long total_chunks, const float* norm_and_coef, double beta1, double beta2, double eps, long long step, void* stream);
/* The same under torch.amp.GradScaler (engine.py:98-106, --amp with fp16: scaler.unscale_ + clip_grad_norm_ + scaler.step, whose
 * found_inf.item() stalls the host every step): the gradients still carry `grad_scale[0]` (device scalar; NULL: already unscaled).
 * amp_state (fp32[6], device): [0] norm of the unscaled gradients, [1] coefficient applied to the scaled gradients = clip / scale,
 * [2] 1 when the step is skipped (non-finite norm, or found_inf[0] != 0 when found_inf is given), [3] number of steps TAKEN (in/out:
 * skipped steps do not advance the bias corrections, as GradScaler skips optimizer.step() as a whole), [4], [5] bias corrections of
 * that count.  ocpg_adamw_step_amp returns without touching p / exp_avg / exp_avg_sq when [2] is set. */
int ocpg_grad_norm_clip_amp(const long long* grads, const long long* numels, const long long* chunk_prefix, int n, long long total_chunks,
                            float max_norm, float* partials, const float* grad_scale, const float* found_inf, double beta1, double beta2,
                            float* amp_state, void* stream);
int ocpg_adamw_step_amp(const long long* params, const long long* grads, const long long* exp_avg, const long long* exp_avg_sq,
                        const long long* numels, const long long* chunk_prefix, const float* lr, const float* weight_decay, int n,
                        long long total_chunks, const float* amp_state, double beta1, double beta2, double eps, void* stream);

/* Classification (sigmoid focal, alpha < 0 disables the alpha weighting) + L1 + GIoU losses of the matched queries, all layers
 * per launch -- replaces SetCriterion.loss_labels / loss_boxes (models/criterion.py:46-107; sigmoid_focal_loss
 * models/segmentation.py:134-160; util/box_ops.py:45-85).  logits [Lr,B,T,Q,K], boxes [Lr,B,T,Q,4] (cxcywh), src [Lr,B] int64
 * matched query, valid [B,T] float, labels [B,T] int64 or NULL, tboxes [B,T,4], num_boxes: device scalar.
 * loss / gloss [3, Lr] = (ce, bbox, giou);  bwd writes glogits and gboxes fully.  bad: optional malformed-box counter. */
int ocpg_det_loss_fwd_f32(const float* logits, const float* boxes, const long long* src, const float* valid, const long long* labels,
                          const float* tboxes, const float* num_boxes, float alpha, int Lr, int B, int T, int Q, int K, float* loss, int* bad,
                          void* stream);
int ocpg_det_loss_bwd_f32(const float* logits, const float* boxes, const long long* src, const float* valid, const long long* labels,
                          const float* tboxes, const float* num_boxes, const float* gloss, float alpha, int Lr, int B, int T, int Q, int K,
                          float* glogits, float* gboxes, void* stream);

/* Spectral gate of LFMResizeAdaptive (models/modules.py:44-50): out [N,2C,h,w] = [Re, Im](X * (1 - coef[n] * high)) for a complex64
 * spectrum X [N,C,h,w] (interleaved re/im), coef [N], high [h*w]; bwd: dX complex [N,C,h,w] fully written, part
 * [N, C * ceil(hw/256)] partial sums with dcoef[n] = sum(part[n]). */
int ocpg_spectral_gate_fwd(const void* X, const float* coef, const float* high, int N, int C, int hw, float* out, void* stream);
/* Channels-last forms of the same block (round 2): the [Re || Im] side as [N, hw, 2C] in the 1x1 convs' compute dtype (0 fp32 /
 * 1 bf16 / 2 fp16), the complex side as [N, C, hw]; 64 x 64 tile transposes through LDS.  c2p = the gate forward (coef, high)
 * or the plain split (coef NULL: the backward of torch.complex(yr, yi), models/modules.py:52-53); p2c = the gate backward
 * (Xs = the saved spectrum: dcoef partials into part [N, ceil(C/64) * ceil(hw/64)]) or the plain merge (Xs, coef NULL). */
int ocpg_spectral_c2p(const void* X, const float* coef, const float* high, int N, int C, int hw, void* pair, int dtype, void* stream);
int ocpg_spectral_p2c(const void* pair, const void* Xs, const float* coef, const float* high, int N, int C, int hw, void* out, float* part,
                      int dtype, void* stream);
int ocpg_spectral_gate_bwd(const float* gout, const void* X, const float* coef, const float* high, int N, int C, int hw, void* dX, float* part,
                           void* stream);

/* Heat-map-weighted cross entropy (masked_ce_loss, models/segmentation.py:177-201, via criterion.py:128-139), all layers:
 * x [Lr, per_layer] logits, w / t [per_layer] = weight map and weighted target of the clip (shared by the layers),
 * per_layer % 4 == 0.  fwd: part [Lr, 512] with loss[l] = sum(part[l]) / per_layer;  bwd: gx [Lr, per_layer] fully written. */
int ocpg_masked_ce_fwd_f32(const float* x, const float* w, const float* t, int Lr, long long per_layer, float* part, void* stream);
int ocpg_masked_ce_bwd_f32(const float* x, const float* w, const float* t, const float* gloss, int Lr, long long per_layer, float* gx,
                           void* stream);

/* Multi-head attention against a SHORT key sequence (Lk <= 32, head_dim 32, H <= 8 with 256 % H == 0) -- replaces the
 * softmax(q k^T * scale + key padding) v core of nn.MultiheadAttention as called by VisionLanguageFusionModule.forward
 * (models/segmentation.py:103-113) and by the decoder layer's self-attention (models/deformable_transformer.py:323-326); the
 * projections around it stay GEMMs.  q [Lq, B, H*32], k / v [Lk, B, H*32], out / dout / dq like q: row (l, b) of tensor X
 * starts at X + (l * B + b) * ldX elements (the projections' own layout, any row stride).  key_pad [B, Lk] bytes, non-zero
 * = ignore this key, or NULL.  pdrop: dropout on the attention weights (0 = off), mask from Philox(seed, offset) keyed on
 * (row, head, key) -- the backward regenerates it.  lse [Lq, B, H] fp32 kept for the backward.  dk / dv [Lk, B, H*32] fp32 are
 * ACCUMULATED into (caller zeroes them).  dtype 0 fp32 / 1 bf16 / 2 fp16 (storage; fp32 arithmetic).
 * Returns -2000 when the shape is not served (the caller keeps its generic attention path). */
int ocpg_attn_smallk_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv,
                         const unsigned char* key_pad, float scale, int Lq, int B, int H, int hd, int Lk, float pdrop,
                         unsigned long long seed, unsigned long long offset, const unsigned long long* rng_base, void* out,
                         long long ldo, float* lse, int dtype, void* stream);
int ocpg_attn_smallk_bwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv,
                         const unsigned char* key_pad, const void* dout, long long ldo, const float* lse, float scale, int Lq,
                         int B, int H, int hd, int Lk, float pdrop, unsigned long long seed, unsigned long long offset,
                         const unsigned long long* rng_base, void* dq, long long lddq, float* dk, float* dv, int dtype, void* stream);

/* The same attention for LONGER key sequences (1 <= Lk <= 128; meant for 33..128, head_dim 32, H <= 8 with 256 % H == 0):
 * csrc/attn_longk.hip walks the keys in chunks of 32 restaged in LDS.  Arguments, layouts, dropout and return codes as for
 * ocpg_attn_smallk_*, except that the dropout stream is indexed (row * H + head) * 128 + key, and that the backward also takes the
 * forward's output `out` (row stride ldout): D = sum_j p~_j dp~_j = dout . out, so one sweep over the keys of a 64-key window suffices;
 * for Lk > 64 the backward is two launches, the second reading and rewriting the dq the first wrote (a 16-bit dq is rounded twice).
 * Lk < 1: -1006;  Lk > 128, hd != 32, H > 8, 256 % H != 0 or B > 65535: -2000 before any HIP call;  Lq == 0 or B == 0: 0. */
int ocpg_attn_longk_fwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv,
                        const unsigned char* key_pad, float scale, int Lq, int B, int H, int hd, int Lk, float pdrop,
                        unsigned long long seed, unsigned long long offset, const unsigned long long* rng_base, void* out,
                        long long ldo, float* lse, int dtype, void* stream);
int ocpg_attn_longk_bwd(const void* q, long long ldq, const void* k, long long ldk, const void* v, long long ldv,
                        const unsigned char* key_pad, const void* dout, long long ldo, const void* out, long long ldout,
                        const float* lse, float scale, int Lq, int B, int H, int hd, int Lk, float pdrop, unsigned long long seed,
                        unsigned long long offset, const unsigned long long* rng_base, void* dq, long long lddq, float* dk, float* dv,
                        int dtype, void* stream);

/* LFM coefficient branch (models/modules.py:17-19,36-39: `self.fc(self.pool(self.laplace(x)))` with laplace a 3x3 VALID conv): the
 * spatial mean of a convolution is linear in the input, mean conv(x)[co] = b[co] + sum w[co,ci,ky,kx] m[ci,ky,kx] with m the mean
 * of x[ci] over the (h-2)x(w-2) window at offset (ky,kx).  x [planes, h, w] fp32 contiguous -> out [planes, 9] window means
 * (as_bf16 != 0: every element is rounded to bf16 first, as the autocast convolution would see it); bwd: gm [planes, 9] ->
 * dx [planes, h, w] fully written. */
/* The LFM block's 2-D Fourier transforms on channels-last maps (csrc/lfm_dft.hip) -- replaces torch.fft.fft2 / ifft2 + the gate / cat /
 * complex / .real / residual chain of LFMResizeAdaptive.forward (models/modules.py:44-56) and their backward:
 *   ocpg_lfm_spectrum_fwd: x real fp32 [N,H,W,C] -> pair [N,H,W,2C] (dtype code pair_dt; channels [0,C) = Re, [C,2C) = Im) =
 *       norm * fft2(x)[n,c,u,v] * (1 - coef[n] * high[u*W+v])   (coef / high NULL: no gate);
 *   ocpg_lfm_spectrum_inv: pair -> out real fp32 [N,H,W,C] = norm * Re(sum_{u,v} pair_c[u,v] * gate * exp(+2 pi i (uy/H + vx/W)))
 *       (+ residual, same layout as out, or NULL); coef_part (or NULL): [N, (W/2+1) * ceil(C/64)] partial sums of
 *       d/dcoef = -sum high * (pair_re * S_re + pair_im * S_im), S = z_saved / gate (z_saved = the forward's gated pair, pair_dt).
 * tmp: scratch of N*H*(W/2+1)*C float2.  Lengths must factor as L1 * L2 with both <= 16 and be <= 128 (ocpg_lfm_dft_supported;
 * ocpg_lfm_dft_split(L) = L1 * 256 + L2, 0 when not served; -2000 from the transforms: the caller keeps the library FFT).
 * tw_h / tw_w: the float2 tables of the length: [0, L) exp(-2 pi i m / L); then the L1-point DFT matrix exp(-2 pi i j k / L1) at
 * [k * L1 + j]; then the L2-point one -- L + L1^2 + L2^2 entries. */
int ocpg_lfm_dft_supported(int H, int W);
int ocpg_lfm_dft_split(int L);
int ocpg_lfm_spectrum_fwd(const float* x, const float* coef, const float* high, int N, int H, int W, int C, const void* tw_h, const void* tw_w,
                          float norm, void* tmp, void* pair, int pair_dt, void* stream);
int ocpg_lfm_spectrum_inv(const void* pair, int pair_dt, const float* coef, const float* high, const void* z_saved, float* coef_part, int N, int H,
                          int W, int C, const void* tw_h, const void* tw_w, float norm, void* tmp, const float* residual, float* out, void* stream);
/* The same two transforms for EVERY length 1 <= H, W <= 256 (csrc/lfm_dft_any.hip): same arguments, same results and layouts as the two
 * entries above, plus the PLAN of each axis by value -- up to three stages whose product is the length, unused stages 1 (anywhere):
 * h1 * h2 * h3 == H, w1 * w2 * w3 == W.  A stage is <= 16, or ONE prime 17..251 per axis (the direct stage; every length <= 256 that
 * is not a product of three stages <= 16 is such a prime times a stage <= 15).  With s0, s1, s2 the stages that are not 1, in the
 * order given (missing ones 1), spectrum element k = k0 + s0 k1 + s0 s1 k2 leaves the line transform in slot (k0 s1 + k1) s2 + k2.
 * tw_h / tw_w: the table of the axis' length L and plan, 2 * E floats + L ints: float2 [0, L) exp(-2 pi i m / L); then, for each stage
 * s <= 16 that is not 1, in plan order, the s-point DFT matrix exp(-2 pi i j k / s) at [k * s + j] (a prime stage above 16 has none:
 * it reads the first table); E = L + the sum of those s^2; then int32 [L]: the slot of spectrum element k.
 * Lengths <= 128 run 64 channels per workgroup, 129..256 run 32: coef_part is [N, (W/2+1) * ceil(C / (H > 128 ? 32 : 64))]; tmp as above.
 * Before any launch, writing nothing: N < 0, H, W, C < 1: -1003 (fwd) / -1007 (inv);  N == 0: 0;  a plan whose product is not the
 * length, a length above 256, a stage < 1, a stage above 16 that is not a prime <= 251, or two such stages on one axis: -2000;  then the
 * null-pointer / dtype codes of the entries above (fwd: x -1001, tw -1005, tmp -1011, pair -1012, coef xor high -1002, pair_dt -1013,
 * N*H or N*(W/2+1) above 2^31-1 -1003; inv: pair -1001, tw -1011, tmp -1014, out -1016, coef xor high -1003, coef_part without coef /
 * z_saved -1005, pair_dt -1002, sizes -1007).  fwd overwrites tmp and every element of pair; inv overwrites tmp, every element of out
 * and, when given, every element of coef_part.  Two launches each, every size by value: capturable. */
int ocpg_lfm_spectrum_fwd_any(const float* x, const float* coef, const float* high, int N, int H, int W, int C, const void* tw_h, const void* tw_w,
                              float norm, void* tmp, void* pair, int pair_dt, int h1, int h2, int h3, int w1, int w2, int w3, void* stream);
int ocpg_lfm_spectrum_inv_any(const void* pair, int pair_dt, const float* coef, const float* high, const void* z_saved, float* coef_part, int N, int H,
                              int W, int C, const void* tw_h, const void* tw_w, float norm, void* tmp, const float* residual, float* out, int h1, int h2,
                              int h3, int w1, int w2, int w3, void* stream);
/* The same two transforms with a CHIRP-Z (Bluestein) line transform on one or both axes (csrc/lfm_dft_czt.hip): the arguments of the _any
 * entries, in their order, plus cz_h / cz_w.  NULL: that axis runs its plan exactly as in the _any entries.  Not NULL: the axis is a chirp
 * axis -- its length L must be 65..128 (prime or not), its plan must be given as (1, 1, L), and the pointer is its table; tw_h / tw_w of a
 * chirp axis is not read but must still not be NULL.  A chirp line is X_k = c_k IFFT_256(FFT_256(a) B)_k with a_n = x_n c_n, c_n =
 * exp(-i pi n^2 / L), B = FFT_256 of conj(c) wrapped around 256 (entry m and entry 256 - m hold conj(c_m), m < L, the rest zero); the
 * inverse direction uses conj(c) and the FFT_256 of the wrapped c.  The table, formed in fp64 by the host, 896 float2:
 *   [0, 128)    c_n for n < L, zero above;
 *   [128, 384)  the forward B divided by 256, in the order the kernel reads it: entry 16 k1 + k2 holds B[k1 + 16 k2];
 *   [384, 640)  the inverse B, the same way;
 *   [640, 896)  exp(-2 pi i m / 256), m < 256.
 * A pass along a chirp axis runs 32 channels per workgroup, so coef_part is [N, (W/2+1) * ceil(C / S)] with S = 32 when H is a chirp
 * axis, else the _any entries' (H > 128 ? 32 : 64); tmp, pair, out, residual, z_saved as above.  Before any launch, writing nothing:
 * the size codes of the _any entries; N == 0: 0; -2000 for a chirp axis outside 65..128, a chirp axis whose plan is not (1, 1, L) and
 * whatever the _any entries refuse of the plan of the other axis; then their null-pointer / dtype codes in their order.  Two launches
 * each, every size by value: capturable. */
int ocpg_lfm_spectrum_fwd_czt(const float* x, const float* coef, const float* high, int N, int H, int W, int C, const void* tw_h, const void* tw_w,
                              float norm, void* tmp, void* pair, int pair_dt, int h1, int h2, int h3, int w1, int w2, int w3, const void* cz_h,
                              const void* cz_w, void* stream);
int ocpg_lfm_spectrum_inv_czt(const void* pair, int pair_dt, const float* coef, const float* high, const void* z_saved, float* coef_part, int N, int H,
                              int W, int C, const void* tw_h, const void* tw_w, float norm, void* tmp, const float* residual, float* out, int h1, int h2,
                              int h3, int w1, int w2, int w3, const void* cz_h, const void* cz_w, void* stream);
int ocpg_window_means3x3_fwd(const float* x, long long planes, int h, int w, int as_bf16, float* out, void* stream);
int ocpg_window_means3x3_bwd(const float* gm, long long planes, int h, int w, float* dx, void* stream);
/* The same on a channels-last map x [N, h, w, C] fp32 (round 4): part [N][ocpg_window_sums3x3_cl_bands(h)][C * 9] = window SUMS of a band of
 * rows (the caller adds the bands and divides by (h-2)(w-2)); bwd_cl: dx [N, h, w, C] = the means' gradient (+ addend, dx's layout, or NULL). */
int ocpg_window_sums3x3_cl_bands(int h);
int ocpg_window_sums3x3_cl(const float* x, int N, int h, int w, int C, int as_bf16, float* part, void* stream);
int ocpg_window_means3x3_bwd_cl(const float* gm, int N, int h, int w, int C, const float* addend, float* dx, void* stream);

/* MSO mask refinement (reference models/decoder.py:14-46; called at models/ocpg.py:375-390 once per decoder layer): all of its
 * convolutions are 3x3 / padding 1 with <= 16 output channels per group, on CHANNELS-LAST maps (csrc/mso.hip).
 *   ocpg_mso_conv3x3   out[n,y,x,o] = sum_{tap,c} w[o][tap][c] * act(in[n,y+dy,x+dx,c]) (+ bias[o]) (+ addend[n % NA,y,x,o]), kept
 *                      where mask[n,y,x,o] > 0 (mask may be NULL), (+ residual[n,y,x,o]).  in [NB,H,W,C] (in_dt), act = ReLU when
 *                      relu_in; w [co_total][9][C] (w_dt; tap = 3 ky + kx); out [NB,H,W,co_total] (out_dt), any co_total (groups
 *                      of 16 output channels).  Forward convolutions AND their input gradients (the same convolution with flipped,
 *                      transposed weights; mask = the input of the ReLU in front of the forward convolution).
 *   ocpg_mso_wgrad     part[band][o][tap][c] = sum over the band's pixels of g[n,y,x,o] * act(x[n,y+dy,x+dx,c]); x [NB,H,W,C]
 *                      (x_dt), g [NB,H,W,co] fp32, co <= 16; bands = NB * ceil(H / rows_per_band), rows_per_band from
 *                      ocpg_mso_wgrad_rows(); the caller sums the bands (the weight gradient).  part_bias (may be NULL)
 *                      [bands][16]: the band's sum of g per output channel (the bias gradient's partial sums).  accumulate != 0:
 *                      part is [co][9][C] and part_bias [16], both ZEROED BY THE CALLER; every band adds its product with float
 *                      atomics (one launch, no reduction pass; the summation order is then not reproducible bit for bit).
 *   ocpg_bilinear_nhwc_fwd / _bwd   F.interpolate(mode="bilinear", align_corners=False, size=(HO, WO)) of a channels-last fp32
 *                      map [NB,H,W,C] (C % 4 == 0) and its input gradient (gather form, fully written, no atomics).
 * compute_dt: 1 / 2 = bf16 / fp16 operands with fp32 accumulation (the autocast convolution), 0 = fp32 operands. */
int ocpg_mso_conv3x3(const void* in, int in_dt, int relu_in, const void* w, int w_dt, const float* bias, const float* addend, int NA,
                     const void* mask, int mask_dt, const float* residual, void* out, int out_dt, int NB, int H, int W, int C,
                     int co_total, int compute_dt, void* stream);
int ocpg_mso_wgrad_rows(int NB, int H, int C, int compute_dt);
int ocpg_mso_wgrad(const void* x, int x_dt, int relu_in, const float* g, float* part, float* part_bias, int accumulate, int NB, int H, int W,
                   int C, int co, int rows_per_band, int compute_dt, void* stream);
int ocpg_bilinear_nhwc_fwd(const float* in, int NB, int H, int W, int C, int HO, int WO, float* out, void* stream);
int ocpg_bilinear_nhwc_bwd(const float* gout, int NB, int H, int W, int C, int HO, int WO, float* gin, void* stream);

/* nn.Linear over FEW rows (decoder layers, box / class heads, controller, LFM coefficient MLPs: models/deformable_transformer.py:
 * 313-336, models/ocpg.py:83-110) under autocast, one launch forward and ONE launch backward (csrc/small_linear.hip):
 *   fwd: y [R, Cout] bf16 = act(x [R, Cin] (fp32 when x_f32 != 0, else bf16) . w [Cout, Cin]^T (bf16) + b [Cout] (bf16 or NULL)),
 *        act = ReLU when relu != 0 (the MLPs' `F.relu(layer(x))`, models/ocpg.py:53-58)
 *   bwd: gx [R, Cin] in x's dtype (NULL: not needed), gw [Cout, Cin] bf16, gb [Cout] bf16 (NULL: no bias) from gy [R, Cout];
 *        y_relu = the forward's output when it applied the ReLU (gy is masked where y <= 0), else NULL
 * Cin must be a multiple of 64 and R <= 4096; otherwise -2000 (the caller keeps its GEMM path).
 * _h16: the same with the 16-bit storage type as an argument (the convention of the conv _h16 symbols): dtype 1 = bfloat16 (the very
 * launch of the un-suffixed symbol, which forwards here), 2 = float16 (the reference's --amp mode: w / b / y / gw / gb / y_relu and a
 * non-fp32 x / gy are fp16, MFMA 32x32x16 f16, fp32 accumulation); any other value returns -1010 before any other check and before
 * anything is launched.  An fp32 x / gy is rounded to nearest-even while it is staged; in fp16 a value past 65504 becomes inf, as ATen's
 * cast makes it (no clamping, no saturation).  Every other check, limit and return code is the un-suffixed symbol's. */
int ocpg_small_linear_fwd(const void* x, int x_f32, const void* w, const void* b, int R, int Cin, int Cout, int relu, void* y, void* stream);
int ocpg_small_linear_bwd(const void* gy, int gy_f32, const void* x, int x_f32, const void* w, const void* y_relu, int R, int Cin, int Cout,
                          void* gx, void* gw, void* gb, void* stream);
int ocpg_small_linear_fwd_h16(const void* x, int x_f32, const void* w, const void* b, int R, int Cin, int Cout, int relu, void* y, int dtype,
                              void* stream);
int ocpg_small_linear_bwd_h16(const void* gy, int gy_f32, const void* x, int x_f32, const void* w, const void* y_relu, int R, int Cin, int Cout,
                              void* gx, void* gw, void* gb, int dtype, void* stream);
/* The same for the fp32 islands (MSDeformAttn's projections over the decoder's few query rows run with autocast disabled, reference
 * models/deformable_transformer.py:329-332): x / w / b / y and every gradient fp32, exact fp32 products on the matrix cores
 * (csrc/small_linear_f32.hip).  gx NULL: not needed; gb NULL: no bias.  Cin % 64 != 0 or R > 4096: -2000. */
int ocpg_small_linear_f32_fwd(const float* x, const float* w, const float* b, int R, int Cin, int Cout, float* y, void* stream);
int ocpg_small_linear_f32_bwd(const float* gy, const float* x, const float* w, int R, int Cin, int Cout, float* gx, float* gw, float* gb, void* stream);

/* nn.LayerNorm over the last axis of a token matrix with low-precision input / output (Video-Swin blocks: norm1, norm2,
 * PatchMerging.norm -- models/video_swin_transformer.py:194,201,225): x [rows, C] with storage code x_f32 (1 fp32, 0 bf16, 2 fp16),
 * gamma / beta fp32 [C], y with storage code y_f32, mean / rstd [rows] fp32 kept for the backward; bwd: dx with code dx_f32, part_g / part_b
 * [ocpg_layernorm_blocks(rows), C] fp32 per-workgroup partial sums of dgamma / dbeta (the caller sums them).  C <= 1024, else -2000. */
int ocpg_layernorm_blocks(long long rows);
int ocpg_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, long long rows, int C, float eps, void* y, int y_f32,
                       float* mean, float* rstd, void* stream);
int ocpg_layernorm_bwd(const void* gy, int gy_f32, const void* x, int x_f32, const float* gamma, const float* mean, const float* rstd,
                       long long rows, int C, void* dx, int dx_f32, float* part_g, float* part_b, void* stream);

/* nn.GroupNorm behind the input projections (models/ocpg.py:108-119: Conv2d -> GroupNorm(32, hidden) per level) between the layouts
 * its neighbours use (csrc/groupnorm.hip): x [N, HW, C] channels-last with storage code x_dtype (1 fp32, 0 bf16, 2 fp16) as the projection
 * GEMM writes it, y [N, C, HW] fp32 planes as the LFM's FFTs read them; gamma / beta fp32 [C]; mean / rstd [N, G] fp32 kept for the backward.
 *   bwd: gy [N, C, HW] fp32 -> dx [N, HW, C] in x's dtype; part [N, 2, C] fp32 = per-frame partial sums of dgamma ([:, 0]) and dbeta ([:, 1]),
 *        summed over N by the caller.
 * Groups of exactly 8 channels (C == 8 G, the reference's 256 / 32), else -2000.  Large maps (C == 256, HW >= 1500) are tiled over pixels
 * and need scratch: work = ocpg_groupnorm_cl_work(N, HW, C, G) floats (0: not needed, work may be NULL); the forward's and the backward's
 * scratch are independent (nothing is carried between the two calls through it). */
long long ocpg_groupnorm_cl_work(long long N, int HW, int C, int G);
int ocpg_groupnorm_cl_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, long long N, int HW, int C, int G, float eps,
                          float* y, float* mean, float* rstd, float* work, void* stream);
int ocpg_groupnorm_cl_bwd(const float* gy, const void* x, int x_dtype, const float* gamma, const float* mean, const float* rstd, long long N,
                          int HW, int C, int G, void* dx, float* part, float* work, void* stream);
/* The same with y / gy channels-last as well ([N, HW, C] fp32; round 4: the LFM's own transforms, csrc/lfm_dft.hip, read that). */
int ocpg_groupnorm_cl2cl_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, long long N, int HW, int C, int G, float eps,
                             float* y, float* mean, float* rstd, float* work, void* stream);
int ocpg_groupnorm_cl2cl_bwd(const float* gy, const void* x, int x_dtype, const float* gamma, const float* mean, const float* rstd, long long N,
                             int HW, int C, int G, void* dx, float* part, float* work, void* stream);

/* Backward of table[idx] ([T, H] -> [M, H]) for a STATIC index (the relative-position-bias lookup, models/video_swin_transformer.py:
 * 112-114,151-153): g [M, H] fp32, order [M] int64 = argsort(idx), seg [T + 1] int64 = CSR offsets of every table row's segment in
 * `order`; out [T, H] fully written.  Segmented sum, no atomics (autograd's index_put(accumulate): ~40 colliding atomics per address). */
int ocpg_gather_rows_bwd(const float* g, const long long* order, const long long* seg, int T, int H, float* out, void* stream);
/* Video-Swin's relative-position bias in the two layouts the window-attention kernels read, straight from the table (round 4) --
 * replaces `relative_position_bias_table[relative_position_index[:N, :N].reshape(-1)].reshape(N, N, -1).permute(2, 0, 1).contiguous()`
 * (models/video_swin_transformer.py:151-153) and the transposed copy: bias[h][a][b] = table[idx[a * ldi + b]][h] (idx: the int64 index
 * buffer, row stride ldi >= N), bias_t = its transpose over (a, b); both fp32 [H, N, N].  bwd: dtable [T, H] from the gradient of
 * `bias` stored [H][N N] (transposed = 0) or from its transpose (transposed != 0: the attention backward's dS sum as it lies);
 * order / seg: positions p = a N + b sorted by idx, segment offsets per table row (T + 1). */
int ocpg_relpos_bias_fwd(const float* table, const long long* idx, int N, long long ldi, int H, float* bias, float* bias_t, void* stream);
int ocpg_relpos_bias_bwd(const float* g, const long long* order, const long long* seg, int T, int H, int N, int transposed, float* out,
                         void* stream);

/* Row gather with padding slots: out [B, M, row] = idx[j] in [0, S) ? x [B, S, row][:, idx[j]] : 0; rows are row_bytes bytes (multiple of
 * 16, any dtype).  Video-Swin's pad + cyclic shift + window partition and its reverse (models/video_swin_transformer.py:171-199) are
 * two such gathers that are each other's backward. */
int ocpg_gather_rows_pad(const void* x, const long long* idx, long long B, long long S, long long M, long long row_bytes, void* out,
                         void* stream);

/* Whole-step HIP-graph capture support (no reference counterpart: the reference launches eagerly).  Replaces every memset node of
 * a captured, not yet instantiated hipGraph_t by a kernel node with the same destination, value, extent and edges: with the HIP
 * runtime of ROCm 7.x a captured hipMemsetAsync writes a stale pattern from the second launch of the instantiated graph on
 * (csrc/graph_util.hip).  *n_replaced (may be NULL) receives the number of nodes rewritten. */
int ocpg_graph_replace_memsets(void* hip_graph, int* n_replaced);
/* Topology of a captured graph: out[9] = nodes, edges, roots, max out-degree, max in-degree, kernel / memset / memcpy / other node
 * counts (a one-stream capture is a chain: roots 1, degrees <= 1). */
int ocpg_graph_stats(void* hip_graph, long long* out9);
/* Memcpy nodes of a captured graph: out[4 i ..] = kind (hipMemcpyKind), bytes, source, destination; returns their number (at most
 * cap are written).  Host-to-device nodes re-read their host source on every replay. */
int ocpg_graph_memcpy_nodes(void* hip_graph, long long* out, int cap);

/* The text gate of VisionLanguageFusionModule (models/segmentation.py:95-113) with its two 256x256 projections folded into the text
 * side (csrc/text_gate.hip): out[b, l, :] = x[b, l, :] * round16(sum_n P[n] V'[b, n, :] + bo), P = per-head
 * softmax over the keys of scale * (round16(x[b, l, :]) . K'[b, n, :] + c[b, n]).  x / g / out / dx [B, L, 256] fp32; K' / V'
 * [B, 8 Lk, 256] in the 16-bit type, c [B, 8 Lk] and bo [256] fp32, rows KEY-major (n = key * 8 + head); key_pad [B, Lk] bytes,
 * non-zero = ignore this key, or NULL.  dtype 1 bf16 / 2 fp16 (the type of K' / V' and of every rounding).
 * Backward: dx, and part [ocpg_text_gate_splits(L)][B][W] fp32 with W = 2 NP 256 + NP + 256, NP = ocpg_text_gate_rows(Lk): per
 * workgroup partial sums over token ranges of dK' [NP][256], dV' [NP][256], dc [NP], dbo [256] (rows past 8 Lk are zero); every
 * element is written, the caller adds the partials over the first axis.  ws: 2 * B * L * NP 16-bit elements of scratch.  No atomics.
 * Served: C = 256, H = 8, 1 <= Lk <= 16, B <= 65535, 16-byte-aligned pointers; anything else returns -2000 before any launch. */
int ocpg_text_gate_rows(int Lk);
int ocpg_text_gate_splits(int L);
int ocpg_text_gate_fwd_h16(const float* x, const void* Kp, const void* Vp, const float* c, const float* bo, const unsigned char* key_pad,
                           float scale, int B, int L, int C, int H, int Lk, float* out, int dtype, void* stream);
int ocpg_text_gate_bwd_h16(const float* x, const float* g, const void* Kp, const void* Vp, const float* c, const float* bo,
                           const unsigned char* key_pad, float scale, int B, int L, int C, int H, int Lk, float* dx, float* part, void* ws,
                           int dtype, void* stream);

/* Inference tail of the mask output (csrc/mask_tail.hip): the stride-4 mask logits straight to what the
 * drivers write -- replaces, per output pixel and with no intermediate tensor, the chain of inference_davis.py:233-261 /
 * inference_ytvos.py (and the eval branch's nearest x4, models/ocpg.py:371-372): nearest x `up`, un-pad crop, bilinear resize to
 * the original size (align_corners=False), sigmoid, then threshold or multi-object merge.
 *   src [K, N, hs, ws] fp32 logits (K objects, N frames).
 *   Virtual map   V[y][x] = src[y / up][x / up] for y < crop_h, x < crop_w; 1 <= crop_h <= hs*up, 1 <= crop_w <= ws*up.
 *   Bilinear      ATen's rule in fp32 and in ATen's operation order: scale = (float)crop / out; s = scale*(d + 0.5f) - 0.5f clamped
 *                 at 0; i0 = (int)s; i1 = i0 + (i0 < crop-1) (against the CROP, not hs*up); l1 = s - i0; l0 = 1 - l1;
 *                 v = l0y*(l0x*a + l1x*b) + l1y*(l0x*c + l1x*d).
 *   Sigmoid       p = 1 / (1 + expf(-v)).
 *   mode 0        out fp32  [N, out_h, out_w] = p.                           K must be 1.
 *   mode 1        out uint8 [N, out_h, out_w] = p > thr ? on_value : 0.      K must be 1; 0 <= on_value <= 255.
 *   mode 2        out uint8 [N, out_h, out_w] = label (inference_davis.py:253-261): p_k < thr becomes 0, candidates [bg, p_1 .. p_K],
 *                 index of the FIRST maximum (ascending scan, strict >: torch.argmax's tie rule).  K <= 255.
 * thr / bg / on_value are ignored by the modes that do not name them.  out is fully overwritten; it needs no alignment beyond its
 * element type's (aligned 16-byte / 4-byte stores are used wherever a lane's 4 pixels allow).  One launch, no atomics, no
 * synchronisation, sizes by value: capturable.
 * Return codes, all before any launch: any size (K, N, hs, ws, up, crop_*, out_*) <= 0: -1006;  mode outside 0..2: -2104;
 * K != 1 in modes 0 / 1: -2101;  K > 255 in mode 2: -2103;  crop_h > hs*up or crop_w > ws*up: -2102;  on_value outside 0..255 in
 * mode 1: -2105;  out_h > 4*65535 or N > 65535 (grid axes): -1008;  src NULL: -1001;  out NULL: -1015. */
int ocpg_mask_tail_f32(const float* src, int K, int N, int hs, int ws, int up, int crop_h, int crop_w, int out_h, int out_w, int mode,
                       float thr, float bg, int on_value, void* out, void* stream);

/* DAVIS-2017 J&F scoring as integer counts (csrc/jf_metrics.hip; reference davis2017/metrics.py:
 * db_eval_iou, f_measure, _seg2bmap).  The fp64 arithmetic on the counts is ocpg_amd/metrics.py:jf_from_counts.
 *   gt, res [T, H, W] uint8 label maps: 0 = background, k = object / proposal k.  Neither pointer needs any alignment.
 *   void_label 0..255: pixels with gt == void_label are removed from both maps, for every pair; -1: none.
 *   Pairs         all_pairs = 0: P = G, pair p = (result id p+1, gt id p+1), R is ignored.
 *                 all_pairs = 1: P = R*G, pair r*G + g = (result id r+1, gt id g+1).
 *   Per pair and frame: A = (res == id_r) & ~void, B = (gt == id_g) & ~void.  Boundary map b(M) (_seg2bmap at equal size; pixels
 *                 outside the image count as 0): y < H-1, x < W-1: (M^M[y,x+1]) | (M^M[y+1,x]) | (M^M[y+1,x+1]);  last row, x < W-1:
 *                 M[H-1,x]^M[H-1,x+1];  last column, y < H-1: M[y,W-1]^M[y+1,W-1];  corner (H-1, W-1): 0.
 *                 A boundary pixel of one map is matched if the other map has a boundary pixel at an in-image offset (dx, dy) with
 *                 dx^2 + dy^2 <= radius^2 (cv2.dilate with skimage.morphology.disk(radius), default border: outside never wins).
 *   counts [P, T, 6] int32, every element overwritten: |A&B|, |A|B|, |b(A)|, |b(B)|, matched pixels of b(A), matched pixels of b(B).
 * Integer arithmetic only: the same result on every call.  A fill kernel zeroes counts (no memset node), one kernel adds per-tile
 * sums with integer atomics (one per workgroup and non-zero count), sizes by value: capturable.
 * Served: 1 <= radius <= 64, G and R <= 254, H*W < 2^31, T <= 65535 and P <= 65535 (grid axes).
 * Return codes, all before any launch: T, H, W, G (or R with all_pairs) <= 0: -1006;  all_pairs outside 0..1: -2201;  radius
 * outside 1..64: -2202;  G (or R with all_pairs) > 254: -2203;  void_label outside -1..255: -2204;  H*W >= 2^31: -2205;  T or P
 * > 65535 or more than 2^31-1 tiles: -1008;  gt or res NULL: -1001;  counts NULL: -1015. */
int ocpg_jf_counts_u8(const unsigned char* gt, const unsigned char* res, int T, int H, int W, int G, int R, int radius, int void_label,
                      int all_pairs, int* counts, void* stream);

/* Weak-annotation similarity head (csrc/sim_heat.hip; reference pre_process/sim_model.py:35-134).
 *   feat [F, h*w, C] fp32, channels contiguous per pixel, 16-byte aligned.  k^_p = feat[f, p] / |feat[f, p]|_2 (an all-zero vector is
 *   outside the contract: the reference divides by zero there).
 *   Objects       obj_frame [n_obj] int32 (device): the frame of object o.  cand_off [n_obj + 1] int32, cand_off[0] = 0, ascending:
 *                 object o owns candidates cand_off[o] .. cand_off[o+1]-1 of cand_xy [total, 2] int32 (device; x, y feature cells,
 *                 0 <= x < w, 0 <= y < h), total = cand_off[n_obj].  cand_off is passed twice: cand_off_host (host memory, validated
 *                 before any launch and used to size the grid) and cand_off (the same numbers in device memory, read by the kernels).
 *   Per candidate c of an object, over the pixels p of the object's frame:  a_c[p] = k^_c . k^_p,
 *                 s_c[p] = (a_c[p] - min_p a_c) / max_p a_c   (divided by the maximum, not the range, as the reference has it).
 *   box NULL      point mode: heat[o] = s of the object's candidate 0, choice[o] = 0, score (if given) = 0.
 *   box [n_obj, 4] int32 (device; x0, y0, x1, y1 feature cells, ends exclusive):  mx[x] = max_y s_c, my[y] = max_x s_c,
 *                 bx[x] = (x0 <= x < x1), by[y] = (y0 <= y < y1),
 *                 score_c = 0.5 * (sum mx*bx / (sum(mx + bx - mx*bx) + 1e-5) + sum my*by / (sum(my + by - my*by) + 1e-5)),
 *                 choice[o] = the candidate (index within the object) of the highest score, the lowest index among equals;
 *                 heat[o] = that candidate's s.
 *   An object without candidates gets a zero plane and choice -1.
 *   heat [n_obj, h, w] fp32 and choice [n_obj] int32 are fully overwritten; score [total] fp32 or NULL.
 *   workspace: ocpg_sim_heat_workspace(F, h, w, total) bytes of device memory, 16-byte aligned (inverse norms [F, h*w], the
 *   similarity rows [total, h*w], per-candidate min / max / score).
 * fp32 in, fp32 accumulate, sums in a fixed order: the same result on every call.  Four launches (norms, rows, per-candidate
 * reduction, selection), no atomics, no memset, plain vector stores only; cells and frames read from device memory are clamped into
 * range before they address anything.
 * Served: C % 4 == 0, h*w <= 8192, at most 256 candidates per object, n_obj <= 65535, F*h*w < 2^31.
 * Return codes, all before any launch: feat NULL or not 16-byte aligned: -1001;  F <= 0: -1002;  h <= 0: -1003;  w <= 0 or
 * h*w > 8192 or F*h*w >= 2^31: -1004;  C <= 0 or C % 4 != 0: -1005;  n_obj <= 0 or > 65535: -1006;  obj_frame NULL: -1007;
 * cand_off_host NULL, cand_off_host[0] != 0, not ascending, or more than 256 candidates in one object: -1008;  cand_off NULL: -1009;
 * cand_xy NULL with total > 0: -1010;  heat NULL: -1012;  choice NULL: -1013;  workspace NULL or not 16-byte aligned: -1015. */
long long ocpg_sim_heat_workspace(int F, int h, int w, int total);
int ocpg_sim_heat_f32(const float* feat, int F, int h, int w, int C, int n_obj, const int* obj_frame, const int* cand_off_host,
                      const int* cand_off, const int* cand_xy, const int* box, float* heat, int* choice, float* score, void* workspace,
                      void* stream);

/* A2D-Sentences / JHMDB-Sentences evaluation as integer counts (csrc/refmask_counts.hip; reference
 * engine.py:126-194, models/postprocessors.py:14-53, datasets/a2d_eval.py).  The fp64 arithmetic on the counts is
 * ocpg_amd/metrics.py: coco_ap_single_gt, RefMaskAccumulator.
 *   src [B, Q, hs, ws] fp32 logits: the annotated frame of each sample, padded to the batch.
 *   Geometry      [B, 4] int32 per sample: crop_h, crop_w (the un-padded augmented size), out_h, out_w (the original size).  Passed
 *                 twice: geom_host (host memory, validated before any launch) and geom (the same numbers in device memory, read by
 *                 the kernel, which clamps them into range again before they address anything).
 *   Ground truth  gt: bytes, non-zero = set; sample b's [out_h, out_w] row-major plane starts at gt + gt_off[b] (gt_off [B] int64 in
 *                 device memory).  No alignment is needed; planes that start on a 4-byte boundary are read 32 bits at a time on
 *                 every row.  Nothing outside a plane's out_h * out_w bytes is read.
 *   Per pixel     exactly ocpg_mask_tail_f32 mode 1: V[y][x] = src[b][q][y / up][x / up] for y < crop_h, x < crop_w; ATen's
 *                 align_corners=False source index in fp32 and in ATen's operation order; the blend; p = 1 / (1 + expf(-v));
 *                 P = p > thr, negated when invert = 1 (the reference's 1 - (sigmoid > 0.5)).
 *   counts [B, Q, 3] int32, every element overwritten: |P & G|, |P|, |G|.
 *   max_out_h / max_out_w: at least every sample's out_h / out_w; they size the grid.
 * Integer arithmetic only: the same result on every call, whatever counts held before.  A fill kernel zeroes counts (no memset
 * node), one kernel adds per-workgroup sums with integer atomics (one per workgroup and non-zero count): capturable.
 * Return codes, all before any launch (counts untouched): B, Q, hs, ws, up, max_out_h, max_out_w or any geometry entry <= 0: -1006;
 * invert outside 0..1: -2301;  crop_h > hs*up or crop_w > ws*up: -2302;  out_h*out_w >= 2^31: -2303;  out_h > max_out_h or
 * out_w > max_out_w: -2304;  geom_host or geom NULL: -2305;  gt or gt_off NULL: -2306;  max_out_h > 4*65535, B*ceil(Q/64) > 65535,
 * hs*up, ws*up or B*Q*3 >= 2^31 (grid axes and index range): -1008;  src NULL: -1001;  counts NULL: -1015. */
int ocpg_refmask_counts_f32(const float* src, int B, int Q, int hs, int ws, int up, const int* geom_host, const int* geom,
                            const unsigned char* gt, const long long* gt_off, int max_out_h, int max_out_w, float thr, int invert,
                            int* counts, void* stream);

/* Everything the matcher and the criterion derive from the batch's targets alone (csrc/target_pack.hip; the
 * torch composition it stands for: models/ops/functions/target_pack_func.py).  B clips of T frames; fp32 unless noted.
 *   Per clip i    masks[i], heat[i], weak[i]: device pointers to dense [T, H_i, W_i] maps (clips may differ in H and W), boxes[i] [T, 4]
 *                 cxcywh, valid[i] [T] int64, labels[i] [T] int64 (labels NULL: no labels), size[i] [2] int64 (h, w).  masks .. size are
 *                 HOST arrays of B device pointers, hw a HOST array [B, 2] of H_i, W_i: the kernels receive them by value, 16 clips per
 *                 launch (no pointer table in device memory, no copy: capturable).
 *   PH, PW        the padded extent (>= every H_i, W_i); pixels past a clip's own extent are zero.  sub(x, k) = x[k/2::k, k/2::k] of the
 *                 padded map.  s, sl: the criterion's strides, sm: the matcher's, (lh, lw): the level-set map size.
 *   gt_s [B,T,PH/s,PW/s] = sub(masks, s);  gt_m [B,T,PH/sm,PW/sm] = sub(masks, sm).
 *   region        the box of frame t on the padded [PH, PW] grid, 1 inside: xyxy = cx -+ 0.5 * w (one rounding), scaled by size
 *                 (w, h, w, h), truncated toward zero; bounds as the Python slice y0:y1, x0:x1 (a negative bound wraps once, then
 *                 clamps to the axis); all zero when the truncated box has no positive width or height.
 *                 region_s [B,T,PH/s,PW/s] = sub(region, s), region_l = sub(region, sl),
 *                 region_ls [B*T, lh, lw] = region_s at rows min(floorf(y * ((float)(PH/s) / lh)), PH/s - 1), columns alike (nearest).
 *   weak_s = sub(weak, s) * region_s, weak_l = sub(weak, sl) * region_l.
 *   w_s, w_l      a = |clamp(sub(heat, k), 0.3, 0.7) - 0.5|, lo / hi = min / max of a over the whole [B,T,..] map,
 *                 (a - lo) / (hi - lo + 1e-5) (IEEE division), 1 where the region is 0.
 *   tboxes [B,T,4] = boxes, valid_f [B,T] fp32 and valid_i [B,T] int64 = valid, labels_out [B,T] int64 = labels.
 *   workspace     ocpg_target_pack_workspace(B) bytes of device memory (per-workgroup min / max).
 * Every output element is written (no pre-zeroing).  ceil(B/16) + 1 launches, no atomics, no memset, the same bits on every call.
 * Served (else -2000, before any launch): PH % k == 0 and PW % (4 * k) == 0 for k = s, sl, sm;  lw % 4 == 0;  T*PH*PW < 2^31.
 * Return codes, all before any launch: B <= 0: -1001;  T <= 0: -1002;  a pointer array or one of its entries NULL: -1003;  H_i or W_i
 * <= 0 or beyond PH / PW: -1004;  PH or PW <= 0: -1005;  a stride <= 0: -1006;  lh or lw <= 0: -1007;  gt_s .. w_l or tboxes NULL or
 * not 16-byte aligned: -1008;  valid_f, valid_i or (with labels) labels_out NULL: -1009;  workspace NULL: -1010. */
long long ocpg_target_pack_workspace(int B);
int ocpg_target_pack_f32(int B, int T, const void* const* masks, const void* const* heat, const void* const* weak, const int* hw,
                         const void* const* boxes, const void* const* valid, const void* const* labels, const void* const* size, int PH,
                         int PW, int s, int sl, int sm, int lh, int lw, float* gt_s, float* gt_m, float* region_s, float* region_l,
                         float* region_ls, float* weak_s, float* weak_l, float* w_s, float* w_l, float* tboxes, float* valid_f,
                         long long* valid_i, long long* labels_out, void* workspace, void* stream);

/* Input front end of a clip (csrc/clip_front.hip): Pillow's 8-bit bilinear Image.resize of a crop window,
 * byte for byte, fused with the horizontal flip, ToTensor + Normalize and the write into a (padded, strided) destination.  Reference:
 * torchvision F.resize on a PIL image (datasets/transforms_video.py) = Image.resize((w, h), BILINEAR) = a horizontal pass, then a
 * vertical pass, each rounded to uint8.
 *   src           P = T*3 uint8 planes of src_h x src_w: plane p, row y, column x at src[p * src_plane + y * src_row + x] (strides in
 *                 bytes; no alignment needed).  The resized image is the window rows top .. top+win_h-1, columns left .. left+win_w-1
 *                 (a crop that was made BEFORE the resize: the taps stop at the window's edges, not the frame's).
 *   Per axis      bounds int32 [out, 2] = (first tap, number of taps) relative to the window, coefs int32 [out, ks] = the taps'
 *                 weights times 2^22, rounded (zero beyond the number of taps); device memory, built on the host in fp64
 *                 (models/ops/functions/clip_front_func.py:resample_tables).  by / ky / ksy: rows; bx / kx / ksx: columns.
 *   Per pass      out = clip_0_255((2^21 + sum_k in[first + k] * coef[k]) >> 22) in int32; the horizontal pass' bytes feed the vertical.
 *   flip          0 / 1: output column x is written to column out_w - 1 - x.
 *   mode 0        dst uint8: the byte.      mode 1        dst fp32: lut[(p % 3) * 256 + byte]  (lut fp32 [3 * 256], device memory).
 *   dst           plane p, row y, column x at dst + p * dst_plane + y * dst_row + x, strides in ELEMENTS.  Exactly out_h x out_w
 *                 elements per plane are written, nothing else (the padding of a batch tensor stays as it is).  Only the element
 *                 type's alignment is needed; 4 elements per store wherever their address allows.
 *   tile_rows     output rows per workgroup, one of 16, 8, 4, 2, 1;  cap_rows: at least the source rows any such tile of tile_rows
 *                 output rows spans (first tap of its first row .. last tap of its last row); cap_rows * 64 bytes of LDS, at most
 *                 32 KiB.  A tile that needs more than cap_rows rows is computed from the first cap_rows (wrong values, no wild access).
 * One launch, integer arithmetic before the table look-up, no atomics, no intermediate in global memory, sizes by value: capturable.
 * Return codes, all before any launch: P, a size or a stride <= 0, ksy / ksx <= 0: -1006;  window outside the frame: -2401;  flip
 * outside 0..1: -2402;  mode outside 0..1: -2403;  tile_rows not one of 16 .. 1: -2404;  cap_rows <= 0 or cap_rows * 64 > 32768: -2405;
 * a table NULL: -2406;  lut NULL in mode 1: -2407;  dst not aligned to its element: -2408;  P > 65535 or more than 65535 row tiles:
 * -1008;  src NULL: -1001;  dst NULL: -1015. */
int ocpg_clip_front_u8(const unsigned char* src, int P, long long src_plane, long long src_row, int src_h, int src_w, int top, int left,
                       int win_h, int win_w, const int* by, const int* ky, int ksy, const int* bx, const int* kx, int ksx, int out_h,
                       int out_w, int flip, int mode, int tile_rows, int cap_rows, void* dst, long long dst_plane, long long dst_row,
                       const float* lut, void* stream);

/* Memory fusion of the mask head, read from the encoder output as it lies (csrc/mask_front.hip; the torch
 * composition it stands for: ocpg.py `sum(bicubic_resize(x.float(), tar) for x in memory)` on the NCHW copies of the memory's levels).
 *   memory [N, S, C] fp32, token-major: level l is an [h_l, w_l, C] channels-last block at token start_l; the levels tile the S tokens.
 *   fusion = x_0 + sum_{1 <= l < n_lvl} My_l x_l Mx_l^T per channel, at level 0's size.
 *   wts           the dense fp32 matrices My_l [h_0, h_l] and Mx_l [w_0, w_l] (resample.bicubic_matrix) of the levels 1 .. n_lvl-1;
 *   rng           int32 pairs (first, count) of the entries of those matrices that are not zero: per output row / column the range of
 *                 source indices (fy [h_0], fx [w_0]) and per source row / column the range of output indices (by [h_l], bx [w_l]).
 *                 The kernels clamp every pair into its axis; entries outside a stated range are taken as zero.
 *   geom_host     HOST array [n_lvl_total, 9] int64: h_l, w_l, start_l, then the offsets of My_l, Mx_l in wts (floats) and of fy, fx,
 *                 by, bx in rng (ints); the offsets of level 0 and of the levels >= n_lvl are not read.  Passed by value to the kernels.
 *   wts_len, rng_len: the elements wts and rng hold (every table is checked to lie inside).
 *   Forward       out_nchw [N, C, h_0, w_0] and out_cl [N, h_0, w_0, C], either may be NULL (not both): the same numbers in two layouts.
 *   Backward      g_nchw / g_cl: the gradients of the two ports, either may be NULL (not both), summed in registers;
 *                 g_memory [N, S, C], every element written: the transposed resampling in gather form for the levels read, zeros for
 *                 the others.  No atomics, sums in a fixed order: the same bits on every call.
 * One launch each, no memset, sizes by value: capturable.
 * Served (else -2000, before any launch): C % 4 == 0; n_lvl_total <= 6; h_l <= h_0 and w_l <= w_0 for the levels read; N <= 65535;
 *   the row tiles fit 64 KiB of LDS (forward 256 * (sum_{l>=1} w_l + w_0 rounded up to 16 k + 1) bytes, backward 272 * w_0).
 * Return codes, all before any launch: memory (forward) NULL or not 16-byte aligned, both gradients NULL or g_cl not aligned
 *   (backward): -1001;  wts or rng NULL with n_lvl > 1: -1002;  geom_host NULL, a size <= 0 or > 65535, levels that do not tile the S
 *   tokens, a table outside wts / rng: -1004;  n_lvl_total < 1 or n_lvl outside 1 .. n_lvl_total: -1005;  N <= 0: -1007;  S <= 0: -1008;
 *   C <= 0: -1009;  both outputs NULL (forward), g_memory NULL or not aligned (backward): -1012;  out_cl not aligned: -1013. */
int ocpg_memfuse_fwd_f32(const float* memory, const float* wts, const int* rng, const long long* geom_host, long long wts_len,
                         long long rng_len, int n_lvl_total, int n_lvl, int N, int S, int C, float* out_nchw, float* out_cl, void* stream);
int ocpg_memfuse_bwd_f32(const float* g_nchw, const float* g_cl, const float* wts, const int* rng, const long long* geom_host,
                         long long wts_len, long long rng_len, int n_lvl_total, int n_lvl, int N, int S, int C, float* g_memory,
                         void* stream);

/* Level-set feature stack of the mask head (csrc/mask_front.hip; the torch lines it stands for: ocpg.py,
 * bilinear x4 of ls_feat_viz's output, sim, the bilinear resize of the frames, cat).
 *   lsf [B*T, h, w, 8] channels-last, fp32 / bf16 / fp16 (lsf_dtype 0 / 1 / 2), 16-byte aligned, widened on load; txt [B, 8] fp32;
 *   frames [B*T, 3, H, W] fp32.  out [B*T, 12, Ho, Wo] fp32, every element written: channels 0-2 the frames and 3-10 lsf, bilinear with
 *   the two-tap tables; 11: sim = (f . t) / (f / max(|f|, 1e-12) . t / max(|t|, 1e-12) + 1e-5) with f = channels 3-10 of the pixel.
 *   tab_i / tab_w  device tables built from resample.bilinear_matrix: per output index the first source index (int) and the two matrix
 *                 entries (float; the second tap is the next index, clamped); by / bx: per source row / column of lsf the (first,
 *                 count) of the fine rows / columns with a non-zero entry.  off_host [12] (host): the int offsets of ly_i [Ho],
 *                 lx_i [Wo], fy_i [Ho], fx_i [Wo], by [h, 2], bx [w, 2] in tab_i, the float offsets of ly_w [Ho, 2], lx_w [Wo, 2],
 *                 fy_w, fx_w in tab_w, and the lengths of tab_i and tab_w.  Every index read from a table is clamped into its axis.
 *   Backward      g [B*T, 12, Ho, Wo] fp32 (channels 0-2 are not read: the frames get no gradient).  g_lsf [B*T, h, w, 8] fp32, every
 *                 element written, gather form; g_txt_part [B, ocpg_lsfeat_bwd_parts(T, Ho, Wo), 8] fp32, every element written: the
 *                 caller sums over the parts.  Channel 11 of g is honoured wherever it is not zero; where it is zero nothing of the sim
 *                 chain is evaluated and the txt gradient is exactly 0.  No atomics: the same bits on every call.
 * One launch each, no memset, sizes by value: capturable.  Served (else -2000): B*T <= 65535, Ho*Wo < 2^31, 8 channels.
 * Return codes, all before any launch: lsf NULL or not aligned: -1001;  lsf_dtype outside 0..2: -1002;  txt NULL: -1003;  a table or
 *   off_host NULL, a table outside tab_i / tab_w: -1004;  B or T <= 0: -1005;  a size <= 0: -1006;  frames (forward) or g (backward)
 *   NULL: -1007;  an output NULL: -1012. */
int ocpg_lsfeat_fwd_f32(const void* lsf, int lsf_dtype, const float* txt, const float* frames, const int* tab_i, const float* tab_w,
                        const long long* off_host, int B, int T, int h, int w, int H, int W, int Ho, int Wo, float* out, void* stream);
int ocpg_lsfeat_bwd_parts(int T, int Ho, int Wo);
int ocpg_lsfeat_bwd_f32(const float* g, const void* lsf, int lsf_dtype, const float* txt, const int* tab_i, const float* tab_w,
                        const long long* off_host, int B, int T, int h, int w, int Ho, int Wo, float* g_lsf, float* g_txt_part,
                        void* stream);

/* Forward of the frozen RoBERTa text encoder (csrc/roberta.hip): fp32 storage and arithmetic, no backward.
 * One launch each, no memset, no workspace, sizes by value: capturable.  No atomics but the integer `bad` counter.
 *
 * ocpg_roberta_embed_ln_f32: out [B, L, C] = LayerNorm(word[ids[b, l]] + type0 + pos[position(b, l)]) with gamma, beta [C], eps.
 *   ids [B, L] int64; word [V, C], pos [P, C], type0 [C] (row 0 of the token-type table); all float tensors 16-byte aligned.
 *   position(b, l) = pad_id + #{j <= l : ids[b, j] != pad_id} where ids[b, l] != pad_id, else pad_id (HF's
 *   create_position_ids_from_input_ids: interior pads do not advance the count); the count is formed inside the kernel.
 *   LayerNorm is two-pass (mean, then the centred sum of squares), one wave per token, the row held in registers.
 *   bad (may be NULL; the caller zeroes it): incremented once per token whose id is outside [0, V); such a token reads no row of
 *   `word`, its word embedding is taken as zeros.  No id makes the kernel read out of bounds.
 *   Served (else -2000): C % 4 == 0 and C <= 1024.  L + pad_id + 1 > P: -2501, nothing is launched (a row of L non-pad tokens would
 *   read past the position table).  Other return codes, all before any launch: a size <= 0 (B, L may be 0: nothing to do) or pad_id
 *   < 0: -1009;  ids NULL: -1001;  word / pos / type0 / gamma / beta NULL or not aligned: -1002 .. -1006;  out: -1014.
 *
 * ocpg_attn_hd64_fwd_f32: out [B, L, H*64] = softmax(q k^T scale + mask) v per (batch, head), head_dim 64.
 *   qkv [B, L, 3, H, 64]: the output of ONE Linear with the stacked q / k / v weights, 16-byte aligned.  attend [B, L], uint8
 *   (attend_i64 0) or int64 (attend_i64 1): non-zero = the key is attended (HF's attention_mask).  A key that is not attended has
 *   probability exactly 0; a query row at such a position is computed like any other.  The score is the 64-term fp32 dot, then scaled.
 *   Every (batch) row must attend at least one key (the caller checks; a row without one yields zeros, not NaN).
 *   Served (else -2000): 1 <= L <= 128, 1 <= H <= 65535, B <= 65535.  One wave per query row, 16 queries per workgroup, K and V of the
 *   (batch, head) in LDS as fp32 with padded rows (L * 133 + 768 floats: 70 KiB at L = 128).
 *   Return codes: a negative size: -1005;  attend_i64 outside 0..1: -1003;  qkv NULL or not aligned: -1001;  attend NULL: -1002;
 *   out NULL: -1008.
 *
 * ocpg_bias_act_f32: y [R, C] = act(x + bias[C]); bias may be NULL; y may BE x (not overlap it otherwise).
 *   act 0: identity;  1: exact GELU 0.5 v (1 + erf(v / sqrt 2));  2: tanh.  4 elements per load / store when x and y are 16-byte aligned.
 *   Return codes: R < 0 or C <= 0: -1003;  act outside 0..2: -1005;  x NULL: -1001;  y NULL: -1006. */
int ocpg_roberta_embed_ln_f32(const long long* ids, const float* word, const float* pos, const float* type0, const float* gamma,
                              const float* beta, float eps, int pad_id, int B, int L, int C, int V, int P, float* out, int* bad,
                              void* stream);
int ocpg_attn_hd64_fwd_f32(const float* qkv, const void* attend, int attend_i64, float scale, int B, int L, int H, float* out,
                           void* stream);
int ocpg_bias_act_f32(const float* x, const float* bias, long long R, int C, int act, float* y, void* stream);

/* COCO run-length encoding of binary masks on the device (csrc/mask_rle.hip): the counts and the compressed
 * string of models/postprocessors.py: rle_counts / rle_encode (the dict pycocotools' `encode` returns), byte for byte.
 *   Format        pixels in COLUMN-major order, k = x * H + y, N = H * W.  Runs alternate 0, 1, 0, ...; the first run is the zeros, of
 *                 length 0 when pixel 0 is set; the last run ends at N.  The string emits count c[i] as x = c[i] - c[i-2] for i > 2
 *                 (from the fourth count on) and as c[i] otherwise, cut into 5-bit groups, low first, as 2's complement; a group is
 *                 the last one when the remaining value is 0 and bit 4 is clear, or -1 and bit 4 is set; other groups carry 0x20;
 *                 every group is offset by 48.  1..7 characters per count.
 *   Two steps, so the call is NOT capturable: the number of runs depends on the data.  Step 1 (one of the two pack entries) writes
 *   the column-major bitmap and per-chunk tables into the workspace and n_trans [n_masks] int32, the transitions of each mask; the
 *   caller reads n_trans back, allocates counts and calls step 2 (ocpg_mask_rle_encode) with the same workspace, n_masks and max_n.
 *   workspace     device memory, 8-byte aligned; max_n >= every mask's H * W.  ocpg_mask_rle_query writes its size in bytes for
 *                 (n_masks, max_n) to *workspace_bytes_host and the chunk size to *chunk_pixels_host (HOST memory, either may be
 *                 NULL): a mask's order is cut into chunks of 4096 pixels, one workgroup each.  The query launches nothing; it
 *                 takes the stream like every entry of the family and does not use it.  The kernels read no word of the workspace
 *                 that they did not write in this call.
 * ocpg_mask_rle_pack_u8: mask m is the row-major [H_m, W_m] byte plane at base + off[m] (off [n_masks] int64, device; no alignment
 *   needed), non-zero = set (torch.bool storage is such a plane).  Geometry [n_masks, 2] int32 = H_m, W_m, passed twice: geom_host
 *   (host memory, validated before any launch) and geom (device memory, read by the kernel and clamped to 1 <= H, H * W <= max_n
 *   before it addresses anything).  Nothing outside a plane's H * W bytes is read.
 * ocpg_mask_rle_pack_logits_f32: the arguments of ocpg_refmask_counts_f32: src [B, Q, hs, ws] fp32, up, geometry [B, 4] int32 =
 *   crop_h, crop_w, out_h, out_w (host and device, clamped likewise).  Mask m = b * Q + q has size out_h[b] x out_w[b]; its pixels
 *   are decided exactly as ocpg_mask_tail_f32 mode 1 decides them (p > thr), negated when invert = 1.  Nothing at the original
 *   resolution is written but the bitmap words.
 * ocpg_mask_rle_encode: run_start [n_masks] int64, passed twice (host: validated; device: read by the kernels and clamped into
 *   0 .. counts_cap): mask m's counts are counts[run_start[m] .. + n_runs[m]), int32, n_runs[m] = n_trans[m] + 1 (int32, device);
 *   its string is the n_bytes[m] (int64, device) characters at bytes + 7 * run_start[m]: bytes holds 7 * counts_cap.
 *   n_trans_host: what step 1 wrote, read back.  Elements of counts and bytes outside a mask's runs / characters are not written.
 * Integer arithmetic only, no atomics, no memset, plain vector stores, no workgroup waits for another: 2 launches per step (pack,
 * per-mask totals; runs, strings).
 * Return codes, all before any launch (nothing written): n_masks, B, Q, hs, ws, up, max_n, counts_cap or a geometry entry <= 0:
 * -1006;  invert outside 0..1: -2601;  geom_host / geom / n_trans_host / run_start_host / run_start NULL: -2605;  crop_h > hs*up or
 * crop_w > ws*up: -2602;  H*W (or max_n) >= 2^31: -2603;  H*W > max_n: -2604;  more than 65535 masks, hs*up or ws*up >= 2^31 (grid
 * axes and index range): -1008;  n_trans_host negative, run starts overlapping, or counts_cap smaller than a mask's start + its
 * n_trans + 1: -2607;  n_trans (pack) or counts / n_runs / bytes / n_bytes (encode) NULL: -1015;  workspace NULL or not 8-byte
 * aligned: -2606;  base, off or src NULL: -1001. */
int ocpg_mask_rle_query(int n_masks, long long max_n, long long* workspace_bytes_host, int* chunk_pixels_host, void* stream);
int ocpg_mask_rle_pack_u8(const unsigned char* base, const long long* off, int n_masks, const int* geom_host, const int* geom,
                          long long max_n, int* n_trans, void* workspace, void* stream);
int ocpg_mask_rle_pack_logits_f32(const float* src, int B, int Q, int hs, int ws, int up, const int* geom_host, const int* geom,
                                  long long max_n, float thr, int invert, int* n_trans, void* workspace, void* stream);
int ocpg_mask_rle_encode(int n_masks, long long max_n, const int* n_trans_host, const long long* run_start_host,
                         const long long* run_start, long long counts_cap, int* counts, int* n_runs, unsigned char* bytes,
                         long long* n_bytes, void* workspace, void* stream);

/* Run-length deflate of 8-bit planes on the device (csrc/png_rle.hip): the deflate stream of a PNG's IDAT
 * chunk for masks and label maps, byte for byte what models/ops/functions/png_func.py composes on the host.
 *   Stream        filter type 0: the filtered data of an H x W plane is H rows of 0x00 + the row's W bytes.  Per row: a fixed-Huffman
 *                 block (BFINAL = 0; the row's tokens; end-of-block) and an empty stored block, so every row ends byte-aligned.  The
 *                 tokens of a row: its W + 1 filtered bytes cut into maximal runs of equal bytes; a run of value v and length n is
 *                 the literal v, (n - 1) / 258 matches of length 258 at distance 1, then one match of length (n - 1) % 258 at
 *                 distance 1 when that is >= 3, that many literals v otherwise.  Behind the last row the final block 03 00.
 *   Two steps, so the call is NOT capturable: the length of a stream depends on the data.
 * ocpg_png_rle_count (2 launches): planes [N, H, W] uint8, contiguous, device, no alignment needed.  Writes the row tables into
 *   workspace (device memory, 8-byte aligned, 24 * N * H bytes) and totals [N, 3] int64 (device, 8-byte aligned): the bytes of plane
 *   m's stream, S0 = sum(d_i) and S1 = sum(i * d_i) over its filtered data d_0 .. d_(n-1), n = H (W + 1), exact in 64 bits.
 *   Adler-32 of the filtered data is ((n + n S0 - S1) mod 65521) << 16 | (1 + S0) mod 65521, to be finished by the caller.
 * ocpg_png_rle_emit (1 launch): the same planes, N, H, W and workspace; totals_host = what step 1 wrote, read back (HOST memory).
 *   The streams are written back to back into out (device, out_cap bytes, no alignment needed): plane m's at the sum of the byte
 *   counts before it.  Bytes of out outside the streams are not written; the kernels read no word of the workspace that they did
 *   not write in this call, clamp what they read of it, and store a row only where it lies inside out_cap.
 * One wave per row, LDS atomic OR into a per-wave bit buffer, plain vector stores, no global atomics, no memset, no workgroup waits
 * for another.
 * Return codes, all before any launch (nothing written): N, H or W <= 0: -1006;  W > 4096 (the per-wave bit buffer): -2701;  N or H
 * > 65535, or N * H > 2^22 rows (grid and the 64-bit bound of S1): -2702;  planes NULL: -1001;  workspace NULL or not 8-byte
 * aligned: -2703;  totals NULL or not 8-byte aligned: -2704;  totals_host NULL or a byte count outside 0 .. H * (9 (W + 1) / 8 + 9):
 * -2705;  out NULL, out_cap <= 0 or smaller than the sum of the byte counts: -2706. */
int ocpg_png_rle_count(const unsigned char* planes, int N, int H, int W, void* workspace, long long* totals, void* stream);
int ocpg_png_rle_emit(const unsigned char* planes, int N, int H, int W, void* workspace, const long long* totals_host,
                      unsigned char* out, long long out_cap, void* stream);

/* library / build identification: returns e.g. "ocpg_hip gfx950 r1" */
const char* ocpg_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OCPG_HIP_H */
