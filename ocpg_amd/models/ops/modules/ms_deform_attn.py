"""MSDeformAttn module -- multi-scale deformable attention around the HIP op.

Same parameters, initialisation and forward contract as the reference's
models/ops/modules/ms_deform_attn.py:31-118 (returns (output, sampling_locations, attention_weights)).
Runs in fp32 regardless of autocast, as the reference does (deformable_transformer.py:250,329) -- unless the caller opts into
16-bit storage of the value path (`value_dtype`; a deviation from the reference, see `resolve_value_dtype`).
"""
import math
import os
import warnings

import torch
import torch.nn.functional as F
from torch import nn

from ... import amp_cache
from ...amp_cache import TokenLinear, linear
from ....util.misc import memo
from ..functions import MSDeformAttnFunction
from ..functions.ms_deform_attn_func import (MSDeformAttnFusedFunction, MSDeformAttnSampleFirstBackwardFunction,
                                              MSDeformAttnSampleFirstFunction)


FUSED_FRONT = os.environ.get("OCPG_MSDA_FUSED_FRONT", "1") != "0"   # A/B switch: softmax + location arithmetic (and their backward) inside the op's kernels
# the same front end for the opt-in 16-bit value path (ocpg_msda_fused_*_h16).  Off unless OCPG_MSDA_FUSED_FRONT_H16 is set to something but "0":
# the 16-bit mode's default stays the un-fused op
FUSED_FRONT_H16 = os.environ.get("OCPG_MSDA_FUSED_FRONT_H16", "0") != "0"
SELECT_PATH = os.environ.get("OCPG_MSDA_SELECT", "1") != "0"     # A/B switch: per-call choice of the grad_value kernel family (self-attention calls)


def sample_first_mode(word):
    """OCPG_MSDA_SAMPLE_FIRST -> "1" (take the sample-first kernels when `sample_first_wanted` says so), "0" (never) or "force" (whenever
    the kernels serve the shape); an unknown word raises ValueError."""
    if word not in ("0", "1", "force"):
        raise ValueError(f"OCPG_MSDA_SAMPLE_FIRST must be one of '0', '1', 'force', not {word!r}")
    return word


# A/B switch: few-query calls sample the unprojected tokens and project the N*Lq*M sampled rows (csrc/msda_sample_first.hip) instead of
# projecting all N*S tokens first
SAMPLE_FIRST = sample_first_mode(os.environ.get("OCPG_MSDA_SAMPLE_FIRST", "1"))
# A/B switch: whether such a call's FORWARD goes through the sample-first kernel too.  Off by default: the forward then keeps value_proj + op
# and `out` keeps its bits (only the backward is the sample-first one).  On, the fp32 summation order of `out` changes (1e-7 relative), which
# under bf16 autocast moves the step's outputs by whole bf16 roundings (measured: DESIGN.md section 4.3c) for another ~70 us per layer
SAMPLE_FIRST_FWD = os.environ.get("OCPG_MSDA_SAMPLE_FIRST_FWD", "0") != "0"
# r of sample_first_wanted: the largest measured 4*Lq*L*P / S at which the kernels were still >= 1.3x faster than value_proj + op with cold
# caches (Lq = 20 at S = 5100: 2.28x; the next point, 0.63, 1.18x -- DESIGN.md section 4.3c, profiles/msda_sample_first_kernel_level.jsonl)
SAMPLE_FIRST_MAX_RATIO = 0.251


def sample_first_wanted(N, S, M, Lq, L, P):
    """Whether a call of this size is worth taking through the sample-first kernels (a pure host function of the sizes):
      * not self-attention (Lq == S reads every value);
      * value_proj is a GEMM over at least amp_cache.TOKEN_LINEAR_MIN_ROWS rows -- below that it is a small GEMM with nothing to win;
      * the 4 * Lq * L * P token rows a head gathers per image are at most SAMPLE_FIRST_MAX_RATIO of the S rows value_proj would write."""
    return Lq != S and N * S >= amp_cache.TOKEN_LINEAR_MIN_ROWS and 4 * Lq * L * P <= SAMPLE_FIRST_MAX_RATIO * S


MERGED_QUERY_PROJ = True      # A/B switch: sampling_offsets and attention_weights as ONE GEMM over the query (they share their input)


_UNSET = object()
_VALUE_DTYPES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16, "autocast": "autocast"}


def resolve_value_dtype(word=None):
    """The module's `value_dtype` for the public switch (args.msda_value_dtype / OCPG_MSDA_VALUE_DTYPE): the argument when it is not
    None, else the environment variable, else "fp32".  -> None (fp32 island, the reference's behaviour), torch.bfloat16, torch.float16,
    or "autocast" (follow torch.get_autocast_dtype("cuda") while autocast is on, fp32 otherwise).  An unknown word raises ValueError."""
    src = "msda_value_dtype"
    if word is None:
        word, src = os.environ.get("OCPG_MSDA_VALUE_DTYPE") or "fp32", "OCPG_MSDA_VALUE_DTYPE"
    if word not in _VALUE_DTYPES:
        raise ValueError(f"{src} must be one of {sorted(_VALUE_DTYPES)}, not {word!r}")
    return _VALUE_DTYPES[word]


def _is_power_of_2(n):
    if not isinstance(n, int) or n < 0:
        raise ValueError(f"invalid input for _is_power_of_2: {n} (type: {type(n)})")
    return n != 0 and (n & (n - 1)) == 0


class MSDeformAttn(nn.Module):
    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4, value_dtype=None):
        """value_dtype: None = the reference's fp32 island.  torch.bfloat16 / torch.float16 (or "autocast": the autocast dtype while
        autocast is on) = 16-bit STORAGE of the value path on the GPU: value_proj, the padding fill, the op's value / output and
        output_proj run in that dtype (fp32 accumulation inside the kernels); the query projections, the softmax, the location arithmetic
        and the returned sampling_locations / attention_weights stay fp32.  Opt-in: not what the reference computes."""
        super().__init__()
        if d_model % n_heads:
            raise ValueError(f"d_model must be divisible by n_heads, but got {d_model} and {n_heads}")
        if not _is_power_of_2(d_model // n_heads):
            warnings.warn("d_model // n_heads should be a power of 2 (the fast HIP kernel needs it; others take the generic kernel)")
        self.im2col_step = 64
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = TokenLinear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = TokenLinear(d_model, n_heads * n_levels * n_points)
        self.value_proj = TokenLinear(d_model, d_model)
        self.output_proj = TokenLinear(d_model, d_model)
        # path-selection state of this module's backward (include/ocpg_hip.h: ocpg_msda_bwd_value_sel_f32): which grad_value kernel family the
        # next call takes, kept on the device by the kernels themselves.  Not part of the state_dict (checkpoints stay interchangeable).
        self.register_buffer("_sel_state", torch.zeros(8, dtype=torch.int32), persistent=False)
        self.set_value_dtype(value_dtype)
        self._reset_parameters()

    def set_value_dtype(self, value_dtype):
        """A CONSTRUCTION-TIME setting (the model builder calls it before the first forward): the owning model caches its fused-cast
        parameter list at its first autocast forward (amp_cache._param_groups), so a change after that would leave value_proj /
        output_proj out of (or stale in) the one-launch cast and the 16-bit path would pay a weight cast per call."""
        if value_dtype not in (None, torch.bfloat16, torch.float16, "autocast"):
            raise ValueError(f"value_dtype must be None, torch.bfloat16, torch.float16 or 'autocast', not {value_dtype!r}")
        self.value_dtype = value_dtype
        if value_dtype is not None:
            # the two value-path projections join the model's one-launch parameter cast (amp_cache.scope): no per-call weight cast
            amp_cache.register(self, self.value_proj.weight, self.value_proj.bias, self.output_proj.weight, self.output_proj.bias)
        else:
            self.__dict__.pop("_amp_cache_extra", None)

    def active_value_dtype(self, x):
        """The 16-bit dtype this call's value path runs in, or None (fp32).  Callers that wrap the module in autocast(enabled=False)
        ask BEFORE they do ("autocast" reads the ambient autocast state) and hand the answer to forward(value_dtype=...)."""
        vd = self.value_dtype
        if vd is None or not x.is_cuda:
            return None
        if vd == "autocast":
            vd = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
            return vd if vd in (torch.bfloat16, torch.float16) else None
        return vd

    @staticmethod
    def _linear16(x, lin, dt):
        w, b = amp_cache.lookup(lin.weight), amp_cache.lookup(lin.bias)
        return linear(x.to(dt), w.to(dt), b.to(dt))          # (.to is the identity for this forward's working copies under matching autocast)

    def _reset_parameters(self):
        """Zero offset/attention weights; offset bias = 8-direction ring scaled by the point index (ms_deform_attn.py:64-78)."""
        nn.init.zeros_(self.sampling_offsets.weight)
        theta = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
        ring = torch.stack([theta.cos(), theta.sin()], -1)
        ring = ring / ring.abs().max(-1, keepdim=True)[0]
        ring = ring.view(self.n_heads, 1, 1, 2).repeat(1, self.n_levels, self.n_points, 1)
        ring = ring * torch.arange(1, self.n_points + 1, dtype=torch.float32).view(1, 1, -1, 1)
        with torch.no_grad():
            self.sampling_offsets.bias = nn.Parameter(ring.reshape(-1))
        nn.init.zeros_(self.attention_weights.weight)
        nn.init.zeros_(self.attention_weights.bias)
        nn.init.xavier_uniform_(self.value_proj.weight)
        nn.init.zeros_(self.value_proj.bias)
        nn.init.xavier_uniform_(self.output_proj.weight)
        nn.init.zeros_(self.output_proj.bias)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None, value_dtype=_UNSET, project_output=True):
        """value_dtype: what a caller that wraps the module in autocast(enabled=False) got from active_value_dtype() (None = fp32);
        left out, the module asks itself.  project_output=False: the first return value is the op's output BEFORE output_proj (the
        caller applies `output_proj_operands` itself, fused with what follows the module)."""
        N, Lq, _ = query.shape
        vd = self.active_value_dtype(input_flatten) if value_dtype is _UNSET else value_dtype
        _, S, _ = input_flatten.shape
        M, L, P = self.n_heads, self.n_levels, self.n_points
        host = getattr(input_spatial_shapes, "_ocpg_host", None)
        if host is not None:
            assert int((host[:, 0] * host[:, 1]).sum()) == S
        else:
            assert (input_spatial_shapes[:, 0] * input_spatial_shapes[:, 1]).sum() == S

        def make_value():
            value = self.value_proj(input_flatten) if vd is None else self._linear16(input_flatten, self.value_proj, vd)
            if input_padding_mask is not None:
                value = value.masked_fill(input_padding_mask[..., None], 0.0)
            return value.view(N, S, M, self.d_model // M)

        # few queries against many tokens (the decoder's cross-attention): value is not formed at all, see below
        sample_first = (vd is None and input_flatten.is_cuda and Lq != S
                        and (SAMPLE_FIRST == "force" or (SAMPLE_FIRST == "1" and sample_first_wanted(N, S, M, Lq, L, P))))
        value = None if sample_first else make_value()
        if MERGED_QUERY_PROJ and query.is_cuda:
            # One GEMM for both query projections (same input, [256 + 128] output columns): one forward GEMM, one input-gradient
            # GEMM and one weight-gradient GEMM instead of two each plus the add of the two input gradients.  With 2-d reference
            # points and host-known level shapes the division of the offsets by (W_l, H_l) is folded into the (tiny) weight:
            # x (W s)^T + b s == (x W^T + b) s column by column -- same products, the scaling moves from 52 MB of offsets to 256 rows.
            n_off = M * L * P * 2
            so_w, so_b = self.sampling_offsets.weight, self.sampling_offsets.bias
            folded = reference_points.shape[-1] == 2 and host is not None
            if folded:
                key = ("msda_inv_wh", tuple(host.flatten().tolist()), M, P)
                inv = memo("msda", key, query.device, lambda: (1.0 / torch.stack([host[:, 1], host[:, 0]], -1).float())[None, :, None, :]
                           .expand(M, L, P, 2).reshape(-1).to(query.device))
                so_w, so_b = so_w * inv[:, None], so_b * inv
            both = linear(query, torch.cat([so_w, self.attention_weights.weight], 0), torch.cat([so_b, self.attention_weights.bias], 0))
            # (each value dtype has its own switch: the fp32 front end is on by default, the 16-bit one is opt-in)
            if ((FUSED_FRONT if vd is None else FUSED_FRONT_H16) and folded and Lq == S
                    and MSDeformAttnFusedFunction.supported(value, both, reference_points, L, P)):
                # lines 96-110 of the reference module inside the kernels: no softmax / add / split-cat passes over the [N, Lq, 384] projection
                out, loc, weights = MSDeformAttnFusedFunction.apply(value.contiguous(), input_spatial_shapes, input_level_start_index, both,
                                                                    reference_points, L, P, self._sel_state if SELECT_PATH else None)
                return self._project(out, vd, project_output), loc, weights
            off2, logit2 = torch.split(both, [n_off, M * L * P], dim=-1)      # split: its backward is ONE cat (two slices: 2 x (zeros + copy) + add)
            offsets = off2.view(N, Lq, M, L, P, 2)
            weights = F.softmax(logit2.view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
        else:
            folded = False
            offsets = self.sampling_offsets(query).view(N, Lq, M, L, P, 2)
            weights = F.softmax(self.attention_weights(query).view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
        if reference_points.shape[-1] == 2:
            if folded:
                loc = reference_points[:, :, None, :, None, :] + offsets
            else:
                wh = torch.stack([input_spatial_shapes[..., 1], input_spatial_shapes[..., 0]], -1)
                loc = reference_points[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
        elif reference_points.shape[-1] == 4:
            loc = reference_points[:, :, None, :, None, :2] + offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
        else:
            raise ValueError(f"Last dim of reference_points must be 2 or 4, but get {reference_points.shape[-1]} instead.")
        loc_c = loc.contiguous()
        if sample_first:
            vp = self.value_proj
            # (without gradients there is no backward to save anything in: the forward-keeping form is today's path then)
            fn = MSDeformAttnSampleFirstFunction if SAMPLE_FIRST_FWD else MSDeformAttnSampleFirstBackwardFunction if torch.is_grad_enabled() else None
            if fn is not None and fn.supported(input_flatten, vp.weight, vp.bias, loc_c, weights):
                out = fn.apply(input_flatten, vp.weight, vp.bias, input_padding_mask, input_spatial_shapes, input_level_start_index, loc_c,
                               weights.contiguous())
                return self._project(out, None, project_output), loc, weights
            value = make_value()          # a shape or dtype the kernels do not serve: today's path
        if SELECT_PATH and Lq == S and loc_c.is_cuda:
            loc_c._ocpg_sel = self._sel_state
        out = MSDeformAttnFunction.apply(value.contiguous(), input_spatial_shapes, input_level_start_index,
                                         loc_c, weights.contiguous(), self.im2col_step)
        return self._project(out, vd, project_output), loc, weights

    def _project(self, out, vd, project_output):
        if not project_output:
            return out
        return self.output_proj(out) if vd is None else self._linear16(out, self.output_proj, vd)

    def output_proj_operands(self, out, vd):
        """(out, weight, bias) of output_proj as the module itself would hand them to amp_cache.linear for this value dtype."""
        lin = self.output_proj
        if vd is None:
            return out, lin.weight, lin.bias
        return out.to(vd), amp_cache.lookup(lin.weight).to(vd), amp_cache.lookup(lin.bias).to(vd)
