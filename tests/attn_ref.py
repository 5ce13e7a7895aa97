"""Key attention (csrc/attn_smallk.hip: 1-32 keys, csrc/attn_longk.hip: 33-128 keys, and 1-128 at its C ABI): an fp64 reference, a
derived ELEMENTWISE error bound, an emulator of the kernels' rounding points with one-line mutants, and the input cases of
tests/test_attn_bounds_cpu.py and tests/test_attn_ref_gpu.py.  Pure torch, CPU or GPU tensors; nothing of the project's is called here.

The assertion of both test files is |got - ref| <= bound for every output element, the bound computed in fp64 from the reference's own
intermediates (`bounds`): no multiplier, no max|ref|, no other kernel's error.

The operation, per batch entry and head (q [Lq, 32], k, v [Lk, 32], g = dout, keep = 0 or 1/(1-pdrop) per weight, 1 without dropout):

    s = scale q k^T (-inf at a padded key)    lse = log sum_j exp s_j    p = exp(s - lse)    p~ = p keep    out = p~ v
    dP~ = g v^T    dP = keep dP~    D = sum_j p_j dP_j (= g . out)    dS = p (dP - D)
    dq = scale dS k    dk = scale dS^T q    dv = p~^T g

Rounding points, read off the kernels.  Both: q, K, V are held in fp32; the forward scales q in fp32 (q * scale is NOT rounded to the
storage type) and takes a 32-term fp32 dot per score; the softmax is online over the keys with __expf, lse = m + __logf(l); out is
acc / l rounded ONCE to storage; dK / dV are fp32 sums over the tokens (registers, then atomics), rounded to storage by the autograd
wrapper only.  Short-key backward: p = __expf(dot(q, k) * scale + bias - lse) (the scale multiplies after the dot), D = sum_j p~_j dp~_j
in fp32, dq rounded once.  Long-key backward: D = dout . out from the STORED, rounded output (a u_st term the short-key kernel does
not have), dq rounded once up to 64 keys and twice beyond (the second window's launch re-reads what the first one wrote).

Notation of `bounds` (first order, running error analysis): u_st the unit roundoff of the storage dtype (2^-8 bf16, 2^-11 fp16, 2^-24
fp32), u32 = 2^-24, c32 the weight given to the fp32 roundings behind one score / one elementary result (a 32-term dot, the scaling,
the exp argument, exp, log, a handful of multiplies: up to ~36 roundings), with the values of tests/win_attn_ref.py: 64 for the 16-bit
cases, above the worst-case count and irrelevant next to u_st; 16 for fp32 storage, which is BELOW the worst-case count: for fp32 the
bound is probabilistic, not a guaranteed first-order one.  It holds as long as the roundings do not all push the same way -- independent
roundings of ~36 terms add to about 6 units rms, and c32 multiplies sums of ABSOLUTE values on top of that -- and a correct kernel
measures at most 0.11 of it; a worst-case fp32 bound would use 64 here as well and lose a factor of 4 in
sensitivity.  e32 = c32 u32; ek = Lk u32 for a chain of Lk fp32 additions over the keys (l, acc, D, dq); `chain` u32 for the longest
chain of additions behind a dK / dV element, from the launch
geometry (`geometry`: 32 tokens per thread and token group, gpb groups per workgroup, then one atomic per thread sharing the address).

    QK      = scale |q| |k|^T                                 (0 at a padded key: its p is exactly 0)
    ds      = e32 (QK + |lse|)                                error of one exp argument s_j - lse, forward or backward
    Dq      = max_j ds_j
    b_lse   = Dq + e32 (|lse| + 1) + ek
    epsP    = ds + sum_i p_i ds_i + e32 + ek                  relative error of a normalised forward probability
    b_out   = (epsP p~) |v| + u_st |out|                      the output rounding
    epsPb   = ds + b_lse + e32                                p recomputed from the stored lse
    bdP~    = e32 (|g| |v|^T)
    bD      = sum_j (epsPb p~ |dP~| + p~ bdP~) + ek sum_j p~ |dP~|          short-key kernel
    bD      = sum_d |g_d| b_out_d + e32 sum_d |g_d| |out_d|                 long-key kernel: the stored output
    bdS     = epsPb p (|dP| + |D|) + p (keep bdP~ + bD)
    b_dq    = scale (bdS |k|) + ek scale (|dS| |k|) + u_st |dq|  [+ u_st |dq of keys 0..63|  long-key kernel past 64 keys]
    b_dk    = scale (bdS^T |q|) + chain u32 scale (|dS|^T |q|) + u_st |dk|
    b_dv    = (epsPb p~)^T |g| + chain u32 (p~^T |g|) + u_st |dv|

(dk / dv leave the C ABI in fp32: `bounds(..., abi=True)` drops the wrapper's u_st |dk| and u_st |dv|, the last fp32 addition being
counted in `chain`; `emulate(..., abi=True)` leaves them unrounded likewise.)

Two absolute floors, both properties of the number formats and not of any kernel (tests/win_attn_ref.py):
  * fp16 storage: 2^-24, the smallest fp16 subnormal, on every bound;
  * every dtype: UNDERFLOW = 2^-100, for probabilities below the smallest normal fp32 number, which fp32 arithmetic may flush.
"""
import collections

import torch

U32 = 2.0 ** -24
U_ST = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
C32 = {torch.bfloat16: 64, torch.float16: 64, torch.float32: 16}
UNDERFLOW = 2.0 ** -100
SCALE = 32 ** -0.5
HD = 32
OUTPUTS = ("out", "lse", "dq", "dk", "dv")
GROSS_MUTANTS = ("dropkey", "padrow", "droptoken", "window2", "groupsum", "lsemax")
CONTRACT_MUTANTS = ("q16", "p16")
MUTANTS = GROSS_MUTANTS + CONTRACT_MUTANTS
# the criterion of test_small_key_attention_kernel / test_long_key_attention_kernel: max|got - ref| <= tol max|ref| + 1e-6
OLD_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-2}

# q = randn * amp, k = randn * kamp.  kamp = 1.5 is what the older tests draw; the peaked cases (amp 3) take 0.75: scores of deviation 2.25
# against 1.5, and the q16 mutant, whose error grows with |s|, stays under the older criterion there too (0.4-0.6 of it in bf16; with
# kamp 1.5 it reaches 1.1-1.7 on dq / dk of those three cases)
Case = collections.namedtuple("Case", "name kernel lq b h lk amp kamp pad pdrop seed")

CASES = [
    Case("s-k1-h1", "short", 7, 3, 1, 1, 1.0, 1.5, "none", 0.0, 101),            # one key, one head, Lq below one token group
    Case("s-k8", "short", 33, 2, 8, 8, 1.0, 1.5, "plan", 0.0, 108),              # backward key bound 8, one token past a group
    Case("s-k9", "short", 33, 2, 8, 9, 1.0, 1.5, "plan", 0.0, 109),
    Case("s-k16-peaked", "short", 70, 2, 4, 16, 3.0, 0.75, "plan", 0.0, 116),     # key bound 16 / 32, peaked softmax
    Case("s-k17-peaked", "short", 70, 2, 4, 17, 3.0, 0.75, "plan", 0.0, 117),
    Case("s-k28", "short", 40, 2, 8, 28, 1.0, 1.5, "plan", 0.0, 128),            # forward LDS 64 640 B
    Case("s-k29", "short", 40, 2, 8, 29, 1.0, 1.5, "plan", 0.0, 129),            # 66 944 B
    Case("s-k32", "short", 40, 2, 8, 32, 1.0, 1.5, "plan", 0.0, 132),            # 73 856 B
    Case("s-k20-h2", "short", 300, 3, 2, 20, 1.0, 1.5, "plan", 0.0, 120),        # two heads, ragged last group
    Case("s-gpb2", "short", 131, 256, 8, 9, 1.0, 1.5, "plan", 0.0, 209),         # gpb 2: 5 groups on 3 workgroups, the last holds one ragged group
    Case("l-k33", "long", 77, 1, 4, 33, 1.0, 1.5, "plan", 0.0, 333),             # one key past the first chunk, that key padded
    Case("l-k64-chunks", "long", 300, 2, 2, 64, 1.0, 1.5, "chunks", 0.0, 364),   # whole first chunk and whole last chunk padded
    Case("l-k65-peaked", "long", 70, 2, 8, 65, 3.0, 0.75, "plan", 0.0, 365),      # second window with a single key, dq rounded twice
    Case("l-k96-h1", "long", 19, 1, 1, 96, 1.0, 1.5, "none", 0.0, 396),          # 2 + 1 chunks, one head
    Case("l-k97", "long", 70, 2, 8, 97, 1.0, 1.5, "plan", 0.0, 397),             # 2 + 2 chunks, one key in the last
    Case("l-k128", "long", 70, 2, 8, 128, 1.0, 1.5, "plan", 0.0, 428),           # the maximum key count
    Case("l-gpb2", "long", 259, 29, 8, 65, 1.0, 1.5, "plan", 0.0, 465),          # gpb 2: 9 groups on 5 workgroups, ragged last, second window
    Case("s-drop", "short", 640, 3, 8, 9, 1.0, 1.5, "none", 0.3, 509),
    Case("l-drop", "long", 200, 2, 4, 70, 1.0, 1.5, "none", 0.3, 570),
]
CASE_IDS = [c.name for c in CASES]


def by_name(name):
    return CASES[CASE_IDS.index(name)]


def round_st(x, dtype):
    return x.to(dtype).to(x.dtype)


def keep_value(pdrop):
    """1 / (1 - pdrop) as the kernels form it: fp32 arithmetic on the fp32 probability."""
    one = torch.ones((), dtype=torch.float32)
    return float(one / (one - torch.tensor(pdrop, dtype=torch.float32)))


def geometry(kernel, lq, b, h, lk):
    """The backward's launch geometry, from the host code of the two .hip files: `tok_per` tokens per token group, `gpb` groups per
    workgroup, `nblocks` workgroups per batch entry, `nparts` threads per (key, channel) address (each adds 32 tokens of a group into its
    register sum and flushes one atomic), `last` groups held by the last workgroup, `windows` (first key, chunks) per launch, and
    `chain`, the longest chain of fp32 additions behind one dK / dV element."""
    tok_per = 256 // h
    groups = (lq + tok_per - 1) // tok_per
    if kernel == "short":
        gpb = 1
        while gpb < 16 and (groups // (2 * gpb)) * b >= 512:
            gpb *= 2
        windows = [(0, 1)]
    else:
        gpb = (groups * b + 255) // 256
        windows = [(0, 1 if lk <= 32 else 2)]
        if lk > 96:
            windows.append((64, 2))
        elif lk > 64:
            windows.append((64, 1))
    nblocks = (groups + gpb - 1) // gpb
    nparts = 8 // h
    return dict(tok_per=tok_per, groups=groups, gpb=gpb, nblocks=nblocks, nparts=nparts, last=groups - (nblocks - 1) * gpb, windows=windows,
                chain=min(32 * gpb, lq) + nparts * nblocks)


def case_geometry(case, kernel=None):
    return geometry(kernel or case.kernel, case.lq, case.b, case.h, case.lk)


def make_pad(case):
    """key_pad [B, Lk] bool or None.  `plan`: entry 0 pads the LAST key (the planted one, see make_inputs), entry 1 pads key 0.
    `chunks` (64 keys): entry 0 pads the whole first chunk and the planted last key, entry 1 pads key 0 and the whole last chunk.
    Every entry keeps a live key."""
    if case.pad == "none":
        return None
    pad = torch.zeros(case.b, case.lk, dtype=torch.bool)
    pad[0, case.lk - 1] = True
    if case.b > 1:
        pad[1, 0] = True
    if case.pad == "chunks":
        pad[0, :32] = True
        pad[1, 32:] = True
    return pad


def why_not(mutant, case):
    """None when `mutant` changes an output of `case`, else the reason why it does not."""
    pad = make_pad(case)
    if mutant == "dropkey":
        if case.lk == 1:
            return "one key: without it the row is empty (NaN, as a fully padded row: out of scope)"
        if pad is not None and bool(pad[:, -1].all()):
            return "the last key is padded for every batch entry already"
    elif mutant == "padrow":
        if case.b == 1:
            return "one batch entry: row 0 is the right row"
        if pad is None or all(torch.equal(pad[i], pad[0]) for i in range(case.b)):
            return "every entry has the padding row of entry 0"
    elif mutant == "window2":
        if case.kernel != "long" or case.lk <= 64:
            return "no second window: the short-key kernel, or at most 64 keys"
    elif mutant == "groupsum":
        if case_geometry(case)["gpb"] == 1:
            return "gpb = 1: a workgroup holds one token group"
    elif mutant in ("q16", "p16"):
        if case.lk == 1:
            return "one key: its probability is 1 whatever the score"
    return None


def mutant_applies(mutant, case):
    return why_not(mutant, case) is None


def make_inputs(case, dtype, keep=None):
    """CPU tensors q, go [Lq, B, C], k, v [Lk, B, C] rounded to `dtype` (held in that dtype), key_pad [B, Lk] bool or None, keep
    [B, H, Lq, Lk] fp32 (0 or 1/(1-p)) or None.  A dropout case without a given `keep` draws one from the case's seed.
    The planted key of a padded case: k[Lk-1, 0] = 4 q[0, 0] -- padded for entry 0, it would take all the weight of token 0 there."""
    lq, b, h, lk = case.lq, case.b, case.h, case.lk
    c = h * HD
    g = torch.Generator().manual_seed(case.seed)
    q = torch.randn(lq, b, c, generator=g) * case.amp
    k = torch.randn(lk, b, c, generator=g) * case.kamp
    v = torch.randn(lk, b, c, generator=g)
    go = torch.randn(lq, b, c, generator=g)
    pad = make_pad(case)
    if pad is not None:
        k[lk - 1, 0] = 4.0 * q[0, 0]
    if case.pdrop > 0 and keep is None:
        keep = (torch.rand(b, h, lq, lk, generator=g) >= case.pdrop).float() * keep_value(case.pdrop)
    return dict(q=q.to(dtype), k=k.to(dtype), v=v.to(dtype), go=go.to(dtype), key_pad=pad, keep=keep, scale=SCALE, h=h)


def _heads(t, h):                    # [L, B, h*32] -> [B, h, L, 32]
    l, b, c = t.shape
    return t.reshape(l, b, h, c // h).permute(1, 2, 0, 3)


def _rows(t):                        # [B, h, L, 32] -> [L, B, h*32]
    b, h, l, hd = t.shape
    return t.permute(2, 0, 1, 3).reshape(l, b, h * hd)


def _T(t):
    return t.transpose(-1, -2)


def reference(q, k, v, go, key_pad, scale, h, keep=None):
    """fp64 on the operands as stored.  Returns the outputs in the kernels' layouts (out, dq [Lq, B, C]; dk, dv [Lk, B, C]; lse
    [Lq, B, H]) and every intermediate in [B, H, Lq | Lk, ...] form."""
    qh, kh, vh, gh = (_heads(t.double(), h) for t in (q, k, v, go))
    b, _, lq, _ = qh.shape
    lk = kh.shape[2]
    live = torch.ones(b, 1, 1, lk, dtype=torch.bool, device=q.device) if key_pad is None else ~key_pad.to(q.device)[:, None, None, :]
    s = (scale * (qh @ _T(kh))).masked_fill(~live, float("-inf"))
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    kp = torch.ones_like(p) if keep is None else keep.double().to(q.device)
    pt = p * kp
    out = pt @ vh
    dPt = gh @ _T(vh)
    dP = kp * dPt
    D = (p * dP).sum(-1, keepdim=True)
    dS = p * (dP - D)
    dq, dk, dv = scale * (dS @ kh), scale * (_T(dS) @ qh), _T(pt) @ gh
    return dict(out=_rows(out), lse=lse[..., 0].permute(2, 0, 1).contiguous(), dq=_rows(dq), dk=_rows(dk), dv=_rows(dv),
                qh=qh, kh=kh, vh=vh, gh=gh, live=live, s=s, lse_h=lse, p=p, keep=kp, pt=pt, out_h=out, dPt=dPt, dP=dP, D=D, dS=dS,
                scale=scale, h=h)


def bounds(R, dtype, kernel, geo, terms=False, abi=False):
    """The elementwise bounds of the module docstring, fp64, shaped like the outputs; `geo` = geometry(...) of the launch.  With `terms`
    also the labelled summands of each bound (for `dominant`: which rounding point a failing element would have to blame).  `abi`: dk / dv
    as they leave the C ABI, in fp32, without the autograd wrapper's rounding to storage."""
    u_st, u32 = U_ST[dtype], U32
    e32 = C32[dtype] * u32
    q, k, v, g, p, pt, kp, scale = R["qh"], R["kh"], R["vh"], R["gh"], R["p"], R["pt"], R["keep"], R["scale"]
    lse, o, dPt, dP, D, dS = R["lse_h"], R["out_h"], R["dPt"], R["dP"], R["D"], R["dS"]
    lk = k.shape[2]
    ek = lk * u32
    chain = geo["chain"] * u32
    live = R["live"].double()
    QK = scale * (q.abs() @ _T(k.abs())) * live
    ds = e32 * (QK + lse.abs()) * live
    Dq = ds.amax(-1, keepdim=True)
    b_lse = Dq + e32 * (lse.abs() + 1) + ek                                    # [B, H, Lq, 1]
    epsP = ds + (p * ds).sum(-1, keepdim=True) + e32 + ek
    t_out = [("probability error epsP", (epsP * pt) @ v.abs()), ("output rounding u_st", u_st * o.abs())]
    b_out = t_out[0][1] + t_out[1][1]
    epsPb = ds + b_lse + e32
    bdPt = e32 * (g.abs() @ _T(v.abs()))
    if kernel == "short":
        bD = (epsPb * pt * dPt.abs() + pt * bdPt).sum(-1, keepdim=True) + ek * (pt * dPt.abs()).sum(-1, keepdim=True)
    else:
        bD = (g.abs() * b_out).sum(-1, keepdim=True) + e32 * (g.abs() * o.abs()).sum(-1, keepdim=True)
    bdS = epsPb * p * (dP.abs() + D.abs()) + p * (kp * bdPt + bD)
    t_lse = [("score error Dq", Dq), ("fp32 roundings e32 (|lse| + 1)", e32 * (lse.abs() + 1)), ("key sum ek", ek + torch.zeros_like(Dq))]
    t_dq = [("dS error", scale * (bdS @ k.abs())), ("key sum ek", ek * scale * (dS.abs() @ k.abs())),
            ("dq rounding u_st", u_st * (scale * (dS @ k)).abs())]
    if kernel == "long" and lk > 64:
        t_dq.append(("rounding of the first window's dq, u_st", u_st * (scale * (dS[..., :64] @ k[:, :, :64])).abs()))
    t_dk = [("dS error", scale * (_T(bdS) @ q.abs())), ("token sum chain u32", chain * scale * (_T(dS.abs()) @ q.abs())),
            ("dk rounding u_st", (0.0 if abi else u_st) * (scale * (_T(dS) @ q)).abs())]
    t_dv = [("probability error epsPb", _T(epsPb * pt) @ g.abs()), ("token sum chain u32", chain * (_T(pt) @ g.abs())),
            ("dv rounding u_st", (0.0 if abi else u_st) * (_T(pt) @ g).abs())]
    lse_rows = lambda t: t[..., 0].permute(2, 0, 1).contiguous()
    T = dict(out=[(n, _rows(t)) for n, t in t_out], lse=[(n, lse_rows(t)) for n, t in t_lse], dq=[(n, _rows(t)) for n, t in t_dq],
             dk=[(n, _rows(t)) for n, t in t_dk], dv=[(n, _rows(t)) for n, t in t_dv])
    floor = UNDERFLOW + (2.0 ** -24 if dtype == torch.float16 else 0.0)
    B = {name: sum(t for _, t in parts) + floor for name, parts in T.items()}
    return (B, T) if terms else B


def dominant(T, name, flat_index):
    """The label of the largest term of output `name`'s bound at one element (T = bounds(..., terms=True)[1])."""
    return max(T[name], key=lambda nt: nt[1].flatten()[flat_index].item())[0]


def emulate(q, k, v, go, key_pad, scale, h, keep=None, kernel="short", mutant=None, abi=False):
    """fp32 torch with the rounding points of `kernel` (the storage dtype is q's); `mutant` plants one defect."""
    dtype = q.dtype
    qh, kh, vh, gh = (_heads(t.float(), h) for t in (q, k, v, go))
    b, _, lq, _ = qh.shape
    lk = kh.shape[2]
    geo = geometry(kernel, lq, b, h, lk)
    ninf = float("-inf")
    pad = torch.zeros(b, lk, dtype=torch.bool) if key_pad is None else key_pad.clone()
    if mutant == "padrow":
        pad = pad[:1].expand(b, lk).clone()
    if mutant == "dropkey":
        pad[:, -1] = True
    dead = pad[:, None, None, :]
    kp = torch.ones(1, dtype=torch.float32) if keep is None else keep.float()
    # forward: q * scale in fp32, online softmax, one rounding of the output
    qs = qh * scale
    if mutant == "q16":
        qs = round_st(qs, dtype)
    s = (qs @ _T(kh)).masked_fill(dead, ninf)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    pf = e / l
    if mutant == "p16":
        pf = round_st(pf, dtype)
    out = round_st((pf * kp) @ vh, dtype)
    # backward: p from the stored lse, the scale behind the dot
    P = torch.exp(((qh @ _T(kh)) * scale).masked_fill(dead, ninf) - lse)
    if mutant == "p16":
        P = round_st(P, dtype)
    Pt = P * kp
    dPt = gh @ _T(vh)
    D = (Pt * dPt).sum(-1, keepdim=True) if kernel == "short" else (gh * out).sum(-1, keepdim=True)
    dS = P * (kp * dPt - D) * scale
    if mutant == "p16":
        dS = round_st(dS, dtype)
    if kernel == "long" and lk > 64:
        dq = round_st(dS[..., :64] @ kh[:, :, :64], dtype)                     # the first launch's dq, stored and re-read
        if mutant != "window2":
            dq = round_st(dq + dS[..., 64:] @ kh[:, :, 64:], dtype)
    else:
        dq = round_st(dS @ kh, dtype)
    tok = torch.arange(lq)
    share = torch.ones(lq)
    if mutant == "droptoken":
        share[-1] = 0.0
    if mutant == "groupsum":
        grp = tok // geo["tok_per"]
        last_of_block = torch.clamp((grp // geo["gpb"] + 1) * geo["gpb"], max=geo["groups"]) - 1
        share = (grp == last_of_block).float()
    share = share[:, None]
    dk, dv = _T(dS * share) @ qh, _T(Pt * share) @ gh
    if not abi:                                                                # the autograd wrapper's rounding
        dk, dv = round_st(dk, dtype), round_st(dv, dtype)
    if mutant == "lsemax":
        lse = torch.log(l)
    return dict(out=_rows(out), lse=lse[..., 0].permute(2, 0, 1).contiguous(), dq=_rows(dq), dk=_rows(dk), dv=_rows(dv))


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


def old_criterion(got, R, dtype):
    """max|got - ref| / (tol max|ref| + 1e-6) per output the older tests read (they do not read lse)."""
    res = {}
    for name in ("out", "dq", "dk", "dv"):
        ref = R[name]
        res[name] = (got[name].detach().double().to(ref.device) - ref).abs().max().item() / (OLD_TOL[dtype] * ref.abs().max().item() + 1e-6)
    return res


def fmt(res):
    return " ".join("%s %.3g" % kv for kv in res.items())


_CACHE = {}


def prepared(case, dtype, device="cpu", keep=None, kernel=None, abi=False):
    """(inputs, reference, bounds) of a case on `device`, computed once per process and never modified by the tests.  `kernel` overrides
    the case's own (the long-key entry points serve short key counts too); a given `keep` replaces the drawn dropout mask."""
    device = torch.device(device)
    kernel = kernel or case.kernel
    rkey = (case.name, dtype, device.type, keep is not None)
    if rkey not in _CACHE:
        inp = make_inputs(case, dtype, keep)
        inp = {name: (x.to(device) if torch.is_tensor(x) else x) for name, x in inp.items()}
        _CACHE[rkey] = (inp, reference(inp["q"], inp["k"], inp["v"], inp["go"], inp["key_pad"], inp["scale"], inp["h"], inp["keep"]))
    inp, R = _CACHE[rkey]
    bkey = rkey + (kernel, abi)
    if bkey not in _CACHE:
        _CACHE[bkey] = bounds(R, dtype, kernel, case_geometry(case, kernel), abi=abi)
    return inp, R, _CACHE[bkey]
