"""Window attention (csrc/win_attn.hip, csrc/win_attn_mfma.hip): an fp64 reference, a derived ELEMENTWISE error bound, an emulator of
the kernels' rounding points with one-line mutants, and the input cases of tests/test_win_attn_bounds_cpu.py and
tests/test_win_attn_ref_gpu.py.  Pure torch, CPU or GPU tensors; nothing of the project's is called here.

The assertion of both test files is |got - ref| <= bound for every output element, the bound computed in fp64 from the reference's own
intermediates (`bounds`): no multiplier, no max|ref|, no other kernel's error.

Notation of `bounds` (first order, running error analysis): u_st the unit roundoff of the storage dtype (2^-8 bf16, 2^-11 fp16, 2^-24
fp32), u32 = 2^-24, c32 an over-count of the fp32 roundings behind one score (a 32-term dot, two adds, the exp argument, the log): 64
for the 16-bit cases, where it is irrelevant next to u_st, 16 for fp32 storage.  With g = dO, dP = g v^T, D = rowsum(g * out),
dS = p (dP - D), dq = scale dS k, dk = scale dS^T q, dv = p^T g:

    QK      = scale * |q| |k|^T
    A       = QK + |bias| + |mask|
    ds      = u_st QK + c32 u32 (A + |lse|)                  q * scale rounded to storage; the fp32 score arithmetic
    Dq      = max_k ds
    b_lse   = Dq + c32 u32 (|lse| + 1)
    epsP    = 2 Dq + c32 u32                                 relative error of a normalised probability
    b_out   = (epsP + 2 u_st) (p |v|) + u_st |out|           P rounded to storage before P V; the output rounding
    epsPb   = 2 Dq + b_lse + c32 u32                         P recomputed from the stored lse
    bD      = rowsum(|g| (b_out + u_st |out|)) + c32 u32 rowsum(|g| |out|)
    bdP     = c32 u32 (|g| |v|^T)
    bdS     = epsPb p (|dP| + |D|) + p (bdP + bD) + u_st |dS|          dS rounded to storage (MFMA operand / the stored dS)
    b_dq    = scale (bdS |k|) + u_st |dq|
    b_dk    = scale (bdS^T |q|) + u_st scale (|dS|^T |q|) + u_st |dk|   the middle term: q re-rounded after scaling
    b_dv    = ((epsPb + u_st) p)^T |g| + u_st |dv|
    b_dbias = sum_bw bdS + c32 u32 sum_bw |dS|
    b_dtable = index_add of b_dbias into the table rows

Two absolute floors, both properties of the number formats and not of any kernel:
  * fp16 storage: 2^-24, the smallest fp16 subnormal, on every bound;
  * every dtype: UNDERFLOW = 2^-100.  A masked pair has p = exp(-100 - ...) ~ 4e-44, below the smallest normal fp32 (and bf16) number
    2^-126: fp32 arithmetic may flush such a value to zero or keep a few bits of it, an ABSOLUTE error of up to 2^-126 per value that
    no relative term covers (an all-masked dbias entry is ~1e-43 with a relative bound of ~1e-45).  An output element is a sum of at
    most BW * N <= 2^12 such values times operands of magnitude <= 2^7 (the planted key is 64): 2^-126 * 2^19 < 2^-100 = 8e-31.  It is
    twenty orders of magnitude below every value a kernel defect could hide in.
"""
import collections

import torch

U32 = 2.0 ** -24
U_ST = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
C32 = {torch.bfloat16: 64, torch.float16: 64, torch.float32: 16}
UNDERFLOW = 2.0 ** -100
SCALE = 32 ** -0.5
OUTPUTS = ("out", "lse", "dqkv", "dbias")
MUTANTS = ("neginf", "biasT", "dropkey", "regionidx")

Case = collections.namedtuple("Case", "name bw nw n h amp kind seed")

CASES = [Case("blocks-n%d" % n, 4, 2, n, 3, 1.0, "blocks", 1000 + n) for n in (1, 31, 32, 33, 64, 65, 129)] + [
    Case("blocks-nw4-n65", 4, 4, 65, 2, 1.0, "blocks", 2065),      # region row 3: split at N - 1, only the last token differs
    Case("peaked-n65", 4, 2, 65, 2, 3.0, "blocks", 3065),
    Case("random-n37", 4, 2, 37, 2, 1.0, "random", 4037),
    Case("none-n33", 2, 1, 33, 1, 3.0, "none", 5033),
    Case("bw1-n33", 1, 1, 33, 2, 1.0, "random", 6033),
]
CASE_IDS = [c.name for c in CASES]


def by_name(name):
    return CASES[CASE_IDS.index(name)]


def has_regions(case):
    return case.kind != "none"


def has_planted_key(case):
    return case.kind == "blocks" and case.nw > 1 and case.n > 2


def mutant_applies(mutant, case):
    if mutant == "neginf":
        return has_planted_key(case)
    if mutant == "regionidx":
        # (NW == 1 or BW == NW: bw // (BW / NW) == bw % NW; N == 1: a token is never masked from itself)
        return has_regions(case) and case.nw > 1 and case.bw > case.nw and case.n > 1
    return case.n > 1                                                         # biasT, dropkey


def round_st(x, dtype):
    return x.to(dtype).to(x.dtype)


def swin_index(window):
    """relative_position_index of a 3-D window (d, h, w), as Video-Swin defines it: [prod(window)] * 2, rows of a
    [(2d-1)(2h-1)(2w-1), heads] table."""
    d, h, w = window
    coords = torch.stack(torch.meshgrid(torch.arange(d), torch.arange(h), torch.arange(w), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += d - 1
    rel[:, :, 1] += h - 1
    rel[:, :, 2] += w - 1
    rel[:, :, 0] *= (2 * h - 1) * (2 * w - 1)
    rel[:, :, 1] *= 2 * w - 1
    return rel.sum(-1)


def table_rows(window):
    return (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)


def make_regions(case):
    if case.kind == "none":
        return None
    nw, n = case.nw, case.n
    region = torch.zeros(nw, n, dtype=torch.int32)
    if case.kind == "blocks":
        for w in range(nw):
            if w % 2 == 0:
                region[w, :] = 5                           # uniform, non-zero: region is non-null and no pair is masked
            else:
                cut = (n // 3, n - 1)[(w // 2) % 2]
                region[w, cut:] = 1 + w
    else:
        g = torch.Generator().manual_seed(case.seed + 1)
        region = torch.randint(0, 3, (nw, n), generator=g).int()
    return region


def make_inputs(case, dtype, index=None, rows=None):
    """CPU tensors: qkv [BW, N, 3, H, 32] and go [BW, N, H*32] rounded to `dtype` (held in that dtype), bias [H, N, N] fp32, region
    [NW, N] int32 or None.  With an index [N, N] into `rows` table rows the bias is table[index] of a table randn * 0.5."""
    bw, nw, n, h = case.bw, case.nw, case.n, case.h
    g = torch.Generator().manual_seed(case.seed)
    qkv = torch.randn(bw, n, 3, h, 32, generator=g) * case.amp
    bias = torch.randn(h, n, n, generator=g) * 0.5
    go = torch.randn(bw, n, h * 32, generator=g)
    table = None
    if index is not None:
        table = torch.randn(rows, h, generator=g) * 0.5
        bias = table[index.reshape(-1)].view(n, n, h).permute(2, 0, 1).contiguous()
    region = make_regions(case)
    if has_planted_key(case):
        # window 1 uses region row 1 (split at N // 3): query 0 lies in the first region, key N - 1 in the other one.  Its raw score
        # 16 * 64 * scale = 181 beats every unmasked key (|score| <= 16 * scale + bias) by more than 100: with the reference's finite
        # -100 it still carries all the weight of query 0, with -inf it carries none.
        qkv[1, 0, 0] = 0.0
        qkv[1, 0, 0, :, 0] = 16.0
        qkv[1, :, 1, :, 0] = qkv[1, :, 1, :, 0].clamp(-1.0, 1.0)
        qkv[1, n - 1, 1, :, 0] = 64.0
    return dict(qkv=qkv.to(dtype), bias=bias, region=region, go=go.to(dtype), table=table, index=index, scale=SCALE, nw=nw)


def _mask(region, bw, nw, value, dtype, rows=None):
    if region is None:
        return None
    if rows is None:
        rows = torch.arange(bw, device=region.device) % nw
    r = region[rows]                                                            # [bw, n]
    differs = r[:, None, :, None] != r[:, None, None, :]
    return torch.zeros(differs.shape, dtype=dtype, device=region.device).masked_fill(differs, value)


def _to_bnc(t):                      # [bw, h, n, 32] -> [bw, n, h*32]
    bw, h, n, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(bw, n, h * hd)


def _from_bnc(t, h):                 # [bw, n, h*32] -> [bw, h, n, 32]
    bw, n, c = t.shape
    return t.reshape(bw, n, h, c // h).permute(0, 2, 1, 3)


def _dtable(dbias, index, rows):
    h, n, _ = dbias.shape
    return torch.zeros(rows, h, dtype=dbias.dtype, device=dbias.device).index_add_(0, index.reshape(-1).to(dbias.device),
                                                                                  dbias.permute(1, 2, 0).reshape(n * n, h))


def reference(qkv, bias, region, scale, nw, go, index=None, rows=None):
    """fp64 on the same storage-rounded inputs; gradients by fp64 autograd of (out * go).sum()."""
    bw, n, _, h, hd = qkv.shape
    a = qkv.double().requires_grad_(True)
    b = bias.double().requires_grad_(True)
    q, k, v = (a[:, :, i].permute(0, 2, 1, 3) for i in range(3))                 # [bw, h, n, hd]
    s = (q * scale) @ k.transpose(-1, -2) + b[None]
    mask = _mask(region, bw, nw, -100.0, torch.float64)
    if mask is not None:
        s = s + mask
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)
    out = _to_bnc(p @ v)
    dqkv, dbias = torch.autograd.grad((out * go.double()).sum(), (a, b))
    R = dict(out=out.detach(), lse=lse.detach(), dqkv=dqkv, dbias=dbias, s=s.detach(), p=p.detach(), q=q.detach(), k=k.detach(),
             v=v.detach(), mask=mask, bias=bias.double(), go=go.double(), scale=scale)
    if index is not None:
        R["dtable"] = _dtable(dbias, index, rows)
    return R


def bounds(R, dtype, index=None, rows=None, c32=None):
    """The elementwise bounds of the module docstring, fp64, shaped like the outputs."""
    u_st, u32 = U_ST[dtype], U32
    c32 = C32[dtype] if c32 is None else c32
    q, k, v, p, scale = R["q"], R["k"], R["v"], R["p"], R["scale"]
    bw, h, n, hd = q.shape
    T = lambda t: t.transpose(-1, -2)
    g = _from_bnc(R["go"], h)
    o = _from_bnc(R["out"], h)
    lse = R["lse"]
    dP = g @ T(v)
    D = (g * o).sum(-1, keepdim=True)
    dS = p * (dP - D)
    dq, dk, dv = scale * (dS @ k), scale * (T(dS) @ q), T(p) @ g
    QK = scale * (q.abs() @ T(k.abs()))
    A = QK + R["bias"].abs()[None] + (R["mask"].abs() if R["mask"] is not None else 0.0)
    ds = u_st * QK + c32 * u32 * (A + lse.abs()[..., None])
    Dq = ds.amax(-1, keepdim=True)                                              # [bw, h, n, 1]
    b_lse = Dq[..., 0] + c32 * u32 * (lse.abs() + 1)
    epsP = 2 * Dq + c32 * u32
    b_out = (epsP + 2 * u_st) * (p @ v.abs()) + u_st * o.abs()
    epsPb = 2 * Dq + b_lse[..., None] + c32 * u32
    bD = (g.abs() * (b_out + u_st * o.abs())).sum(-1, keepdim=True) + c32 * u32 * (g.abs() * o.abs()).sum(-1, keepdim=True)
    bdP = c32 * u32 * (g.abs() @ T(v.abs()))
    bdS = epsPb * p * (dP.abs() + D.abs()) + p * (bdP + bD) + u_st * dS.abs()
    b_dq = scale * (bdS @ k.abs()) + u_st * dq.abs()
    b_dk = scale * (T(bdS) @ q.abs()) + u_st * scale * (T(dS.abs()) @ q.abs()) + u_st * dk.abs()
    b_dv = T((epsPb + u_st) * p) @ g.abs() + u_st * dv.abs()
    b_dbias = bdS.sum(0) + c32 * u32 * dS.abs().sum(0)
    B = dict(out=_to_bnc(b_out), lse=b_lse, dqkv=torch.stack([b_dq, b_dk, b_dv], 0).permute(1, 3, 0, 2, 4), dbias=b_dbias)
    if index is not None:
        B["dtable"] = _dtable(b_dbias, index, rows)
    floor = UNDERFLOW + (2.0 ** -24 if dtype == torch.float16 else 0.0)
    return {name: b + floor for name, b in B.items()}


def emulate(qkv, bias, region, scale, nw, go, index=None, rows=None, mutant=None):
    """fp32 torch with the kernels' rounding points (the storage dtype is qkv's); `mutant` plants one defect."""
    dtype = qkv.dtype
    bw, n, _, h, hd = qkv.shape
    T = lambda t: t.transpose(-1, -2)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).float() for i in range(3))
    g = _from_bnc(go.float(), h)
    qs = round_st(q * scale, dtype)
    b = bias.float()
    if mutant == "biasT":
        b = T(b)
    s = qs @ T(k) + b[None]
    if region is not None:
        region_rows = torch.arange(bw) // (bw // nw) if mutant == "regionidx" else None
        s = s + _mask(region, bw, nw, -float("inf") if mutant == "neginf" else -100.0, torch.float32, region_rows)
    if mutant == "dropkey":
        s[..., -1] = -float("inf")
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    out = round_st((round_st(p, dtype) @ v) / l, dtype)
    lse = m + torch.log(l)
    P = torch.exp(s - lse)
    D = (g * out).sum(-1, keepdim=True)
    dSr = round_st(P * (g @ T(v) - D), dtype)
    dq = round_st(scale * (dSr @ k), dtype)
    dk = round_st(T(dSr) @ qs, dtype)
    dv = round_st(T(round_st(P, dtype)) @ g, dtype)
    E = dict(out=_to_bnc(out), lse=lse[..., 0], dqkv=torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4), dbias=dSr.sum(0))
    if index is not None:
        E["dtable"] = _dtable(E["dbias"], index, rows)
    return E


def ratios(got, R, B):
    """Worst |got - ref| / bound per output present in `got` (a non-finite value counts as inf)."""
    res = {}
    for name, x in got.items():
        ref, bound = R[name], B[name]
        x = x.detach().double().to(ref.device)
        assert x.shape == ref.shape, (name, tuple(x.shape), tuple(ref.shape))
        r = (x - ref).abs() / bound
        r = torch.where(torch.isfinite(x), r, torch.full_like(r, float("inf")))
        res[name] = r.max().item()
    return res


def fmt(res):
    return " ".join("%s %.3g" % kv for kv in res.items())


_CACHE = {}


def prepared(case, dtype, index=None, rows=None):
    """(inputs, reference, bounds) of a case, computed once per process on the CPU and never modified by the tests."""
    key = (case.name, dtype, index is not None)
    if key not in _CACHE:
        inp = make_inputs(case, dtype, index, rows)
        R = reference(inp["qkv"], inp["bias"], inp["region"], inp["scale"], inp["nw"], inp["go"], index, rows)
        _CACHE[key] = (inp, R, bounds(R, dtype, index, rows))
    return _CACHE[key]
