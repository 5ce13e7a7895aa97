"""Autograd bindings of csrc/fused_ln.hip: LayerNorm(res + dropout(x)) and dropout(relu(x W^T + b)) as single passes.

The dropout masks are never stored: forward and backward evaluate the same counter-based generator on (seed, offset);
seed = torch.initial_seed() (so torch.manual_seed governs it), offset = a per-process call counter.  The counter is
state OUTSIDE torch's generators: util/checkpoint.py saves / restores it (get_rng_state / set_rng_state below), so a resumed
run continues the mask sequence instead of replaying it from offset 1.

HIP graphs: a captured launch bakes its by-value arguments into the node, so a replayed step would draw the SAME masks every
time.  Calls made while a `GraphRng` is active therefore also hand the kernels a DEVICE pointer to a per-capture base word that
the kernel adds to its offset; the captured step ends with `advance()` (base += calls per replay, one tiny captured kernel), so
replay r of a graph captured at host counter c0 uses offsets c0 + r * J + j -- exactly the offsets eager step r would have used
(tests/test_graph_gpu.py: consecutive replays differ, replay k == eager step k).
"""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ...._lib import DTYPE_CODE as _DT, check, lib
from .gemm_func import mm

# A/B switch, read once: the extra ports of the dropout+add+LayerNorm kernels (y + addend and a 16-bit copy of y forward, up to three
# gradient addends and the Linear's bias-gradient partials backward) and the Linear + dropout/add/LN autograd node; 0 = the plain calls
PORTS = os.environ.get("OCPG_FUSED_LN_PORTS", "1") != "0"
# A/B switch, read once: the encoder FFN's bias + ReLU + dropout passes as epilogues of own MFMA GEMMs (csrc/gemm_dgrad_bn.hip, bf16, from
# amp_cache.TOKEN_LINEAR_MIN_ROWS rows).  fwd: linear1 + ocpg_bias_relu_dropout_fwd = ocpg_gemm_bias_relu_dropout_fwd;  bwd: linear2's input
# gradient (formed in LinearDropoutAddLayerNorm.backward) + ocpg_bias_relu_dropout_bwd = ocpg_gemm_dgrad_mask.  0 | fwd | bwd | 1 (both).
# OCPG_FFN_FWD_EXACT (default 0): 1 = the fused forward adds the bias BEFORE the GEMM result is rounded to bf16 (one rounding fewer);
# 0 = it rounds first, as the pair does.  The exact form decides ReLUs of pre-activations within a bf16 spacing of zero the other way than
# the pair, which moves the step's outputs by more than a rounding, so it is opt-in.
_FFN_FUSED = os.environ.get("OCPG_FFN_FUSED", "1")
FFN_FWD_EXACT = os.environ.get("OCPG_FFN_FWD_EXACT", "0") != "0"
if _FFN_FUSED not in ("0", "fwd", "bwd", "1"):
    raise RuntimeError(f"OCPG_FFN_FUSED={_FFN_FUSED}: expected 0, fwd, bwd or 1")
FFN_FUSED_FWD, FFN_FUSED_BWD = _FFN_FUSED in ("1", "fwd"), _FFN_FUSED in ("1", "bwd")
FFN_TILE = 0                # 128 x 128, the fastest tile at the encoder's shapes (tools/bench_ffn_fused.py)
FFN_TILE_ROWS = (128, 64, 64)       # rows of a workgroup tile (csrc/gemm_dgrad_bn.hip TILE_M): one row of partial column sums per row tile
_FFN_DECLINED = (-2000, -2001, -2002)       # shape / alignment / dtype the fused symbols do not serve: the caller keeps the pair
_calls = [0]
_active = [None]            # the GraphRng whose capture is in progress (at most one per process)


class GraphRng:
    """Per-capture device state of the dropout generator: state[0] = base added to every captured call's offset when the
    kernel runs, state[1] = calls per replay.  Use:  `with rng: <capture, ending with rng.advance()>`, then `rng.finalize()`
    once after the capture and `rng.replayed()` after every replay (keeps the host counter, which checkpoints save, in step)."""

    def __init__(self, device):
        self.state = torch.zeros(2, dtype=torch.int64, device=device)
        self.c0, self.calls = None, 0

    def __enter__(self):
        assert _active[0] is None, "nested graph captures of the dropout generator"
        self.c0 = _calls[0]
        _active[0] = self
        return self

    def __exit__(self, *exc):
        self.calls = _calls[0] - self.c0
        _calls[0] = self.c0         # a capture executes nothing: the first replay is the step that uses offsets c0 + 1 ...
        _active[0] = None
        return False

    def advance(self):
        """LAST operation inside the capture: base += calls per replay (state[1] is filled by finalize())."""
        self.state[0:1].add_(self.state[1:2])

    def finalize(self):
        self.state[1] = self.calls

    def replayed(self):
        _calls[0] += self.calls


def _rng():
    """(seed, offset, base pointer or None) of the next dropout call."""
    _calls[0] += 1
    g = _active[0]
    return torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, _calls[0], (None if g is None else g.state.data_ptr())


def _unpack(rng):
    """Explicit generators (tests): (seed, offset) or (seed, offset, base pointer)."""
    rng = rng if rng is not None else _rng()
    return (rng[0], rng[1], rng[2] if len(rng) > 2 else None)


def get_rng_state():
    return {"dropout_calls": _calls[0]}


def set_rng_state(state):
    _calls[0] = int(state.get("dropout_calls", 0))


def _st():
    return torch.cuda.current_stream().cuda_stream


class DropoutAddLayerNorm(Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, p, eps, rng):
        c = x.shape[-1]
        x2, res2 = x.reshape(-1, c).contiguous(), res.reshape(-1, c).contiguous()
        r = x2.shape[0]
        seed, offset, base = _unpack(rng)
        y = torch.empty((r, c), dtype=torch.float32, device=x.device)
        stats = torch.empty((2, r), dtype=torch.float32, device=x.device)
        check(lib().ocpg_dropout_add_ln_fwd(x2.data_ptr(), res2.data_ptr(), gamma.data_ptr(), beta.data_ptr(), r, c, float(eps), float(p), seed,
                                            offset, base, _DT[x2.dtype], y.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), _st()),
              "ocpg_dropout_add_ln_fwd")
        ctx.save_for_backward(x2, res2, gamma, stats)
        ctx.meta = (float(p), seed, offset, base, x.shape, res.shape)
        return y.view(res.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x2, res2, gamma, stats = ctx.saved_tensors
        p, seed, offset, base, xshape, rshape = ctx.meta
        r, c = x2.shape
        gy = gy.reshape(r, c).float().contiguous()
        gx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        gres = torch.empty_like(res2) if ctx.needs_input_grad[1] else None
        part = torch.empty((lib().ocpg_dropout_add_ln_bwd_slots(r), 2, c), dtype=torch.float32, device=x2.device)
        check(lib().ocpg_dropout_add_ln_bwd(gy.data_ptr(), x2.data_ptr(), res2.data_ptr(), gamma.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
                                            r, c, p, seed, offset, base, _DT[x2.dtype], None if gx is None else gx.data_ptr(),
                                            None if gres is None else gres.data_ptr(), part.data_ptr(), _st()),
              "ocpg_dropout_add_ln_bwd")
        dgb = part.sum(0)
        return (None if gx is None else gx.view(xshape), None if gres is None else gres.view(rshape), dgb[0], dgb[1], None, None, None)


def _dal_fwd_ex(x2, res2, gamma, beta, p, eps, seed, offset, base, addend, lp_dtype):
    """-> (y, stats, y_add | None, y_lp | None): the forward kernel with its extra ports"""
    r, c = x2.shape
    y = torch.empty((r, c), dtype=torch.float32, device=x2.device)
    stats = torch.empty((2, r), dtype=torch.float32, device=x2.device)
    y_add = torch.empty_like(y) if addend is not None else None
    y_lp = torch.empty((r, c), dtype=lp_dtype, device=x2.device) if lp_dtype is not None else None
    check(lib().ocpg_dropout_add_ln_fwd_ex(x2.data_ptr(), res2.data_ptr(), gamma.data_ptr(), beta.data_ptr(), r, c, float(eps), float(p), seed,
                                           offset, base, _DT[x2.dtype], y.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
                                           None if addend is None else addend.data_ptr(), None if y_add is None else y_add.data_ptr(),
                                           None if y_lp is None else y_lp.data_ptr(), 0 if lp_dtype is None else _DT[lp_dtype], _st()),
          "ocpg_dropout_add_ln_fwd_ex")
    return y, stats, y_add, y_lp


def _dal_bwd_ex(grads, x2, res2, gamma, stats, p, seed, offset, base, want_gx, want_gres, want_gxsum):
    """grads: the gradients of (y, y_add, y_lp) that arrived (1..3 tensors [R, C], fp32 / bf16 / fp16), summed inside the kernel
    -> (gx | None, gres | None, dgb_part, gxsum_part | None)"""
    r, c = x2.shape
    gs = []
    for g in grads:
        g = g.reshape(r, c)
        if g.dtype not in _DT:
            g = g.float()
        gs.append(g if g.is_contiguous() else g.contiguous())
    gs += [None] * (3 - len(gs))
    gx = torch.empty_like(x2) if want_gx else None
    gres = torch.empty_like(res2) if want_gres else None
    slots = lib().ocpg_dropout_add_ln_bwd_slots(r)
    part = torch.empty((slots, 2, c), dtype=torch.float32, device=x2.device)
    gxsum = torch.empty((slots, c), dtype=torch.float32, device=x2.device) if want_gxsum else None
    ga = []
    for g in gs:
        ga += [None, 0] if g is None else [g.data_ptr(), _DT[g.dtype]]
    check(lib().ocpg_dropout_add_ln_bwd_ex(*ga, x2.data_ptr(), res2.data_ptr(), gamma.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
                                           r, c, p, seed, offset, base, _DT[x2.dtype], None if gx is None else gx.data_ptr(),
                                           None if gres is None else gres.data_ptr(), part.data_ptr(),
                                           None if gxsum is None else gxsum.data_ptr(), _st()),
          "ocpg_dropout_add_ln_bwd_ex")
    return gx, gres, part, gxsum


class DropoutAddLayerNormPorts(Function):
    """DropoutAddLayerNorm with the kernels' extra ports: -> (y, y + addend | None, y in lp_dtype | None).  The backward hands the
    gradients that arrived for the three outputs to the kernel as they are (no cast, no add); an output nobody used is skipped."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, p, eps, rng, addend, lp_dtype):
        c = x.shape[-1]
        x2, res2 = x.reshape(-1, c).contiguous(), res.reshape(-1, c).contiguous()
        ad2 = None if addend is None else addend.reshape(-1, c).contiguous()
        seed, offset, base = _unpack(rng)
        y, stats, y_add, y_lp = _dal_fwd_ex(x2, res2, gamma, beta, p, eps, seed, offset, base, ad2, lp_dtype)
        ctx.save_for_backward(x2, res2, gamma, stats)
        ctx.meta = (float(p), seed, offset, base, x.shape, res.shape, None if addend is None else addend.shape)
        ctx.set_materialize_grads(False)
        return y.view(res.shape), None if y_add is None else y_add.view(res.shape), None if y_lp is None else y_lp.view(res.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gadd, glp):
        x2, res2, gamma, stats = ctx.saved_tensors
        p, seed, offset, base, xshape, rshape, ashape = ctx.meta
        grads = [g for g in (gy, gadd, glp) if g is not None]
        if not grads:
            return (None,) * 9
        gx, gres, part, _ = _dal_bwd_ex(grads, x2, res2, gamma, stats, p, seed, offset, base, ctx.needs_input_grad[0], ctx.needs_input_grad[1], False)
        dgb = part.sum(0)
        ga = gadd.reshape(ashape) if (gadd is not None and ctx.needs_input_grad[7]) else None
        return (None if gx is None else gx.view(xshape), None if gres is None else gres.view(rshape), dgb[0], dgb[1], None, None, None, ga, None)


class LinearDropoutAddLayerNorm(Function):
    """LayerNorm(res + dropout(x2 W^T + b)) as ONE autograd node, for a Linear over many rows (amp_cache.TokenLinearFunction's GEMMs):
    forward = GEMM with its bias epilogue + the dropout/add/LN kernel; backward = that kernel's backward, which also leaves the partial
    column sums of the Linear's output gradient (its bias gradient), then the input-gradient GEMM and the row-split weight gradient."""

    @staticmethod
    def forward(ctx, x2, w, b, res, gamma, beta, p, eps, rng, addend, lp_dtype):
        from ...amp_cache import deferrable
        from .conv_bn_func import _claim_token
        h = mm(x2, w, True, b)
        c = h.shape[-1]
        # consumer: x2 IS a LinearBiasReluDropout output whose bias + ReLU + dropout backward this node's input-gradient GEMM can take over
        ctx.claim = _claim_token(x2) if (FFN_FUSED_BWD and x2.dtype == torch.bfloat16 and w.dtype == x2.dtype and x2.is_contiguous()
                                         and w.is_contiguous() and ctx.needs_input_grad[0]) else None
        res2 = res.reshape(-1, c).contiguous()
        ad2 = None if addend is None else addend.reshape(-1, c).contiguous()
        seed, offset, base = _unpack(rng)
        y, stats, y_add, y_lp = _dal_fwd_ex(h, res2, gamma, beta, p, eps, seed, offset, base, ad2, lp_dtype)
        ctx.save_for_backward(x2, w, h, res2, gamma, stats)
        ctx.meta = (float(p), seed, offset, base, res.shape, None if addend is None else addend.shape)
        ctx.has_bias = b is not None
        ctx.defer_w, ctx.defer_b = deferrable(w), b is not None and deferrable(b) and b.dtype == h.dtype
        ctx.set_materialize_grads(False)
        return y.view(res.shape), None if y_add is None else y_add.view(res.shape), None if y_lp is None else y_lp.view(res.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gadd, glp):
        from ...amp_cache import defer_sum, weight_grad
        x2, w, h, res2, gamma, stats = ctx.saved_tensors
        p, seed, offset, base, rshape, ashape = ctx.meta
        grads = [g for g in (gy, gadd, glp) if g is not None]
        if not grads:
            return (None,) * 11
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gh, gres, part, gxsum = _dal_bwd_ex(grads, h, res2, gamma, stats, p, seed, offset, base, True, ctx.needs_input_grad[3], need_b)
        dgb = part.sum(0)
        gb = None
        if need_b:
            gb = defer_sum(gxsum, h.dtype) if (ctx.defer_b and h.dtype != torch.float32) else gxsum.sum(0).to(h.dtype)
        gx = None
        if ctx.claim is not None and ctx.needs_input_grad[0]:
            gx = _ffn_dgrad_mask(gh, w, x2, ctx.claim)
        if gx is None and ctx.needs_input_grad[0]:
            gx = mm(gh, w)
        gw = weight_grad(gh, x2, ctx.defer_w) if ctx.needs_input_grad[1] else None
        ga = gadd.reshape(ashape) if (gadd is not None and ctx.needs_input_grad[9]) else None
        return (gx, gw, gb, None if gres is None else gres.view(rshape), dgb[0], dgb[1], None, None, None, ga, None)


def _ffn_rows_ok(r):
    from ... import amp_cache
    return r >= amp_cache.TOKEN_LINEAR_MIN_ROWS


def _ffn_dgrad_mask(gh, w, h, tok):
    """gx [R, N] = (gh [R, K] w [K, N]) * scale * [h > 0] by ocpg_gemm_dgrad_mask, the partial column sums parked on the producer's token;
    None when the symbol declines (nothing written: the caller runs its GEMM and the producer its own backward pass)."""
    r, k = gh.shape
    n = w.shape[1]
    if gh.dtype != h.dtype or not gh.is_contiguous() or tuple(w.shape) != (k, n) or tuple(h.shape) != (r, n) or not _ffn_rows_ok(r):
        return None
    L = lib()
    gx = torch.empty_like(h)
    tm = FFN_TILE_ROWS[FFN_TILE]
    part = torch.empty(((r + tm - 1) // tm, n), dtype=torch.float32, device=h.device)      # one row of column sums per row tile
    rc = L.ocpg_gemm_dgrad_mask(gh.data_ptr(), w.data_ptr(), h.data_ptr(), tok["scale"], gx.data_ptr(), part.data_ptr(), r, n, k, _DT[h.dtype],
                                FFN_TILE, _st())
    if rc in _FFN_DECLINED:
        return None
    check(rc, "ocpg_gemm_dgrad_mask")
    from .conv_bn_func import _fill_token
    _fill_token(tok, gx, part)
    return gx


class LinearBiasReluDropout(Function):
    @staticmethod
    def forward(ctx, x2, w, b, p, rng, splits):
        seed, offset, base = _unpack(rng)
        r, c = x2.shape[0], w.shape[0]
        h = None
        if (FFN_FUSED_FWD and x2.dtype == torch.bfloat16 and w.dtype == x2.dtype and b.dtype == x2.dtype and _ffn_rows_ok(r)
                and x2.is_contiguous() and w.is_contiguous() and b.is_contiguous()):
            h = torch.empty((r, c), dtype=x2.dtype, device=x2.device)
            rc = lib().ocpg_gemm_bias_relu_dropout_fwd(x2.data_ptr(), w.data_ptr(), b.data_ptr(), float(p), seed, offset, base, h.data_ptr(), r, c,
                                                       x2.shape[1], _DT[x2.dtype], FFN_TILE, 0 if FFN_FWD_EXACT else 1, _st())
            if rc in _FFN_DECLINED:
                h = None
            else:
                check(rc, "ocpg_gemm_bias_relu_dropout_fwd")
        if h is None:
            h = mm(x2, w, True)
            check(lib().ocpg_bias_relu_dropout_fwd(h.data_ptr(), b.data_ptr(), r, c, float(p), seed, offset, base, _DT[h.dtype], h.data_ptr(), _st()),
                  "ocpg_bias_relu_dropout_fwd")
        ctx.save_for_backward(x2, w, h)
        ctx.meta = (float(p), splits)
        from ...amp_cache import deferrable
        ctx.defer_w, ctx.defer_b = deferrable(w), deferrable(b) and b.dtype == h.dtype
        # producer: the consumer whose input IS h (linear2 inside LinearDropoutAddLayerNorm) may apply this node's bias + ReLU + dropout
        # backward in its input-gradient GEMM and leave the bias gradient's partial column sums on the token
        ctx.offer = None
        if FFN_FUSED_BWD and h.dtype == torch.bfloat16 and _ffn_rows_ok(r) and any(ctx.needs_input_grad[:3]):
            from .conv_bn_func import _offer_token
            ctx.offer = _offer_token(h, 1.0 / (1.0 - float(p)), False, "OCPG_FFN_FUSED", "Linear + bias + ReLU + dropout")
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, gh):
        from ...amp_cache import weight_grad
        x2, w, h = ctx.saved_tensors
        p, splits = ctx.meta
        r, c = h.shape
        from .conv_bn_func import _take_token
        fused = _take_token(ctx.offer, gh)
        if fused is not None:       # linear2's input-gradient GEMM already applied this node's backward pass: gh IS ga
            ga, part = fused
        else:
            gh = gh.to(h.dtype).contiguous()
            ga = torch.empty_like(h)
            slots = lib().ocpg_bias_relu_dropout_bwd_slots(r, c, _DT[h.dtype])
            part = torch.empty((slots, c), dtype=torch.float32, device=h.device)
            check(lib().ocpg_bias_relu_dropout_bwd(gh.data_ptr(), h.data_ptr(), r, c, p, _DT[h.dtype], ga.data_ptr(), part.data_ptr(), _st()),
                  "ocpg_bias_relu_dropout_bwd")
        from ...amp_cache import defer_sum
        # the per-slot partial column sums: summed inside the fused gradient cast when the bias copy allows it (one launch less + no cast)
        dbias = defer_sum(part, h.dtype) if (ctx.defer_b and ctx.needs_input_grad[2] and h.dtype != torch.float32) else part.sum(0).to(h.dtype)
        gx = mm(ga, w) if ctx.needs_input_grad[0] else None
        gw = weight_grad(ga, x2, ctx.defer_w) if ctx.needs_input_grad[1] else None
        return gx, gw, dbias if ctx.needs_input_grad[2] else None, None, None, None


def supported(x, res, c):
    return (x.is_cuda and x.dtype in _DT and res.dtype == torch.float32 and c % 4 == 0 and c <= 2048 and x.shape == res.shape)


def dropout_add_layer_norm_ports(x, res, norm, p, addend=None, lp_dtype=None, rng=None):
    """-> (norm(res + dropout_p(x)) fp32, that + addend (fp32, or None), that in lp_dtype (bf16 / fp16, or None)): one pass each way."""
    return DropoutAddLayerNormPorts.apply(x, res, norm.weight, norm.bias, p, norm.eps, rng, addend, lp_dtype)


def linear_dropout_add_layer_norm(x2, w, b, res, norm, p, addend=None, lp_dtype=None, rng=None):
    """The same three outputs for x = x2 W^T + b (x2 [R, K], w, b of one dtype): Linear + dropout/add/LN as one autograd node."""
    return LinearDropoutAddLayerNorm.apply(x2, w, b, res, norm.weight, norm.bias, p, norm.eps, rng, addend, lp_dtype)


def dropout_add_layer_norm(x, res, norm, p, rng=None):
    """norm(res + dropout_p(x)) for an nn.LayerNorm over the last axis; res fp32, x fp32/bf16; -> fp32."""
    return DropoutAddLayerNorm.apply(x, res, norm.weight, norm.bias, p, norm.eps, rng)
