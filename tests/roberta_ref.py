"""The native RoBERTa text encoder (ocpg_amd/models/text_encoder/roberta_native.py, csrc/roberta.hip): an fp64 referee of the whole
encoder, fp64 references of its three kernels and a derived ELEMENTWISE error bound for each.  Pure torch on CPU tensors; nothing of the
project's is called here, and HF transformers only to build seeded random modules (`tiny_model`).

The referee (`encoder`) restates the arithmetic of the runner's docstring on a state dict widened to fp64:

    position ids   pad + #{j <= l : ids[b, j] != pad} where ids[b, l] != pad, else pad
    x = LN(word[ids] + pos[position ids] + type[0])
    per layer:     a = attention(x Wq^T + bq, x Wk^T + bk, x Wv^T + bv), scale 1/sqrt(64) = head_dim^-1/2, keys with mask 0 at -inf
                   x = LN(a Wo^T + bo + x);   h = gelu_erf(x W1^T + b1);   x = LN(h W2^T + b2 + x)
    pooler = tanh(x[:, 0] Wp^T + bp)

Kernel bounds: |got - ref| <= bound for every output element, the bound computed in fp64 from the reference's own intermediates, first
order, every constant a COUNT of roundings read off the kernel (u32 = 2^-24, the unit roundoff of fp32) or a documented accuracy of an
instruction / library function:

embed_layer_norm (one wave per token, the row in registers):
    z = (w + t) + p                   two roundings:  dz = u32 (|w + t| + |z|)
    mean: a lane adds its 4 nch values (nch = ceil(C / 256) float4 per lane), 6 shuffle additions, 1 division:  row = 4 nch + 6 + 1
    b_mean = row u32 mean|z| + mean(dz)
    d = z - mean:  dd = dz + u32 |d|
    b_var  = 2 mean(|d| dd) + mean((dd + b_mean)^2) + (row + 1) u32 var        two-pass: the mean's error enters squared
    rstd = rsqrtf(var + eps):  the addition (1), the division by C is counted in row + 1, v_rsq_f32 is a 1-ulp instruction (2 u32), one
           spare for the conversion of C:  K_RS = 4 (the same count as tests/norm_ref.py);   rel_rs = b_var rstd^2 / 2 + K_RS u32
    xhat = (z - mean) rstd:  the subtraction and the product, E = 2;  y = xhat gamma + beta: the product and the addition, E = 2
    b_xhat = rstd (b_mean + dz) + |xhat| (rel_rs + 2 u32)
    b_y    = |gamma| b_xhat + 2 u32 (|xhat gamma| + |beta|)
  A token whose id is outside [0, V) has w = 0 (and is counted in `bad`).

attention_hd64 (one wave per query; lanes = keys for the scores, = channels for the output):
    s_j = fl(sum_d q_d k_jd) scale     a 64-term fma chain (each partial sum rounded once) and the product:  ds_j = (64 + 1) u32 scale |q| . |k_j|
    t_j = s_j - m, m = max_j s_j       the common shift cancels in p = e / l, only the subtraction's rounding stays:  u32 |t_j|
    e_j = __expf(t_j) = v_exp_f32(t_j log2 e):  the product and the rounded constant move the argument by at most 2 u32 |t_j| (relative
          error of e_j, as d/dt e^t = e^t), the instruction is accurate to 1 ulp = 2 u32:   ee_j = (2 |t_j| + 2) u32
    eps_j = ds_j + u32 |t_j| + ee_j                                             relative error of e_j
    l = sum_j e_j:  p0 + p1, then 6 shuffle additions of positive terms:  7 u32
    epsP_j = eps_j + sum_i p_i eps_i + 7 u32                                    relative error of p_j = e_j / l
    acc_d = sum_j e_j v_jd:  a chain of L fmas:  L u32 sum_j p_j |v_jd|;   out = acc / l:  one correctly rounded division, u32 |out|
    b_out = sum_j epsP_j p_j |v_jd| + L u32 sum_j p_j |v_jd| + u32 |out| + 2^-126 sum_j |v_jd|
  The last term is a property of the format: an e_j below the smallest normal fp32 number may be flushed to zero.  A key that is not
  attended has p = 0 exactly and appears in no term.

bias_act:
    z = x + b  one rounding, dz = u32 |z| (0 without a bias)
    none:  b = dz
    gelu:  y = (0.5 z) (1 + erf(z c)), c = fl(1 / sqrt 2).  0.5 z is exact; z c: the product and the rounded constant, 2 u32 |z c| on erf's
           argument, times erf' = 2 / sqrt pi exp(-(z c)^2);  erff: ERF_ULP = 16 ulp, the accuracy the OpenCL specification requires of erf and
           the device library (OCML) documents as its contract, 1 ulp = 2 u32 of |erf|;  1 + erf: u32 |1 + erf|;  the last product: u32 |y|;
           the input rounding through gelu'(z) = Phi(z) + z phi(z):
           b = 0.5 |z| (2 ERF_ULP u32 |erf| + erf'(zc) 2 u32 |z c| + u32 |1 + erf|) + u32 |y| + |gelu'(z)| dz + 2^-126
    tanh:  tanhf: TANH_ULP = 5 ulp (the same source), b = 2 TANH_ULP u32 |y| + (1 - y^2) dz + 2^-126
"""
import math

import torch

U32 = 2.0 ** -24
K_RS = 4
ERF_ULP = 16
TANH_ULP = 5
FLT_MIN = 2.0 ** -126
HEAD_DIM = 64
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------------- models
def tiny_config(**over):
    from transformers import RobertaConfig
    kw = dict(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=40,
              type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0, eos_token_id=2)
    kw.update(over)
    return RobertaConfig(**kw)


def base2_config():
    """RoBERTa-base's shape cut to 2 layers and a 1000-word vocabulary"""
    return tiny_config(vocab_size=1000, hidden_size=768, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=514)


def seeded_model(cfg, seed=0):
    """A random-initialised HF RobertaModel in eval mode; every parameter drawn from the seed (biases and LayerNorm parameters too, so
    that none of them is a silent 0 / 1)."""
    from transformers import RobertaModel
    g = torch.Generator().manual_seed(seed)
    m = RobertaModel(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return m.eval()


def padded_ids(b, l, vocab, seed, pad=1):
    """ids [b, l] with <s> ... </s> and trailing pads of different lengths per row (row 0 full), attention_mask = ids != pad."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (b, l), generator=g)
    ids[:, 0] = 0
    for r in range(b):
        n = max(2, l - (r * l) // (2 * max(b - 1, 1))) if r else l
        ids[r, n - 1] = 2
        ids[r, n:] = pad
    return ids, ids.ne(pad).long()


# ------------------------------------------------------------------------------------------------------------------------ referee
def position_ids(ids, pad):
    out = torch.full_like(ids, pad)
    for b in range(ids.shape[0]):
        n = 0
        for l in range(ids.shape[1]):
            if int(ids[b, l]) != pad:
                n += 1
                out[b, l] = pad + n
    return out


def layer_norm(z, gamma, beta, eps):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + eps) * gamma + beta


def gelu_erf(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def attention(q, k, v, attend, heads, scale):
    """q, k, v [B, L, H * 64] fp64, attend [B, L] (non-zero = attended) -> [B, L, H * 64]"""
    b, l, c = q.shape
    sp = lambda t: t.reshape(b, l, heads, c // heads).permute(0, 2, 1, 3)
    s = (sp(q) @ sp(k).transpose(-1, -2)) * scale
    s = s.masked_fill(attend.eq(0)[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ sp(v)).permute(0, 2, 1, 3).reshape(b, l, c)


def encoder(state_dict, ids, attention_mask, heads, eps, pad, layers=None):
    """The fp64 referee -> (last_hidden_state [B, L, C], pooler_output [B, C]); state_dict: an HF RobertaModel's (any float dtype)."""
    sd = {k: v.to(F64) for k, v in state_dict.items() if v.is_floating_point()}
    lin = lambda x, name: x @ sd[name + ".weight"].t() + sd[name + ".bias"]
    ln = lambda z, name: layer_norm(z, sd[name + ".weight"], sd[name + ".bias"], eps)
    x = sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.position_embeddings.weight"][position_ids(ids, pad)] \
        + sd["embeddings.token_type_embeddings.weight"][0]
    x = ln(x, "embeddings.LayerNorm")
    if layers is None:
        layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
    for i in range(layers):
        p = f"encoder.layer.{i}."
        a = attention(lin(x, p + "attention.self.query"), lin(x, p + "attention.self.key"), lin(x, p + "attention.self.value"), attention_mask,
                      heads, HEAD_DIM ** -0.5)
        x = ln(lin(a, p + "attention.output.dense") + x, p + "attention.output.LayerNorm")
        h = gelu_erf(lin(x, p + "intermediate.dense"))
        x = ln(lin(h, p + "output.dense") + x, p + "output.LayerNorm")
    return x, torch.tanh(lin(x[:, 0], "pooler.dense"))


def referee_of(model, ids, attention_mask):
    cfg = model.config
    assert cfg.hidden_size == cfg.num_attention_heads * HEAD_DIM
    return encoder(model.state_dict(), ids, attention_mask, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.pad_token_id)


def hf_forward(model, ids, attention_mask):
    with torch.no_grad():
        enc = model(input_ids=ids, attention_mask=attention_mask)
    return enc.last_hidden_state, enc.pooler_output


def max_err(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


# ---------------------------------------------------------------------------------------------------- kernel references and bounds
def embed_reference(ids, word, pos, type0, gamma, beta, eps, pad):
    """-> (y, bound, bad): fp64 reference of embed_layer_norm on fp32 tables (widened), its elementwise bound, the out-of-range count"""
    word, pos, type0, gamma, beta = (t.to(F64) for t in (word, pos, type0, gamma, beta))
    v, c = word.shape
    ok = (ids >= 0) & (ids < v)
    w = word[ids.clamp(0, v - 1)] * ok[..., None].to(F64)
    p = pos[position_ids(ids, pad)]
    wt = w + type0
    z = wt + p
    rmean = lambda t: t.mean(-1, keepdim=True)
    mean = rmean(z)
    d = z - mean
    var = rmean(d * d)
    rstd = (var + eps) ** -0.5
    xhat = d * rstd
    y = xhat * gamma + beta
    nch = (c // 4 + 63) // 64
    row = 4 * nch + 6 + 1
    dz = U32 * (wt.abs() + z.abs())
    b_mean = row * U32 * rmean(z.abs()) + rmean(dz)
    dd = dz + U32 * d.abs()
    b_var = 2 * rmean(d.abs() * dd) + rmean((dd + b_mean) ** 2) + (row + 1) * U32 * var
    rel_rs = 0.5 * b_var * rstd ** 2 + K_RS * U32
    b_xhat = rstd * (b_mean + dz) + xhat.abs() * (rel_rs + 2 * U32)
    b_y = gamma.abs() * b_xhat + 2 * U32 * ((xhat * gamma).abs() + beta.abs())
    return y, b_y, int((~ok).sum())


def attention_reference(qkv, attend, heads, scale):
    """qkv [B, L, 3, H, 64] fp32, attend [B, L] -> (out [B, L, H * 64] fp64, bound)"""
    b, l = qkv.shape[:2]
    q, k, v = qkv.to(F64).reshape(b, l, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)             # [B, H, L, 64]
    live = attend.ne(0)[:, None, None, :]
    lf = live.to(F64)
    s = (q @ k.transpose(-1, -2)) * scale
    sm = s.masked_fill(~live, float("-inf"))
    m = sm.amax(-1, keepdim=True)
    t = torch.where(live, s - m, torch.zeros_like(s))
    p = torch.softmax(sm, -1)
    out = p @ v
    ds = (HEAD_DIM + 1) * U32 * scale * (q.abs() @ k.abs().transpose(-1, -2))
    eps_j = (ds + U32 * t.abs() + (2 * t.abs() + 2) * U32) * lf
    epsP = eps_j + (p * eps_j).sum(-1, keepdim=True) + 7 * U32
    bound = (epsP * p) @ v.abs() + l * U32 * (p @ v.abs()) + U32 * out.abs() + FLT_MIN * (lf.expand_as(p) @ v.abs())
    pack = lambda x: x.permute(0, 2, 1, 3).reshape(b, l, heads * HEAD_DIM)
    return pack(out), pack(bound)


def bias_act_reference(x, bias, act):
    """x [R, C] fp32, bias [C] fp32 or None -> (y fp64, bound)"""
    z = x.to(F64) + (0 if bias is None else bias.to(F64))
    dz = U32 * z.abs() if bias is not None else torch.zeros_like(z)
    if act == "none":
        return z, dz
    if act == "tanh":
        y = torch.tanh(z)
        return y, 2 * TANH_ULP * U32 * y.abs() + (1 - y * y) * dz + FLT_MIN
    assert act == "gelu"
    a = z / math.sqrt(2.0)
    erf = torch.erf(a)
    derf = 2.0 / math.sqrt(math.pi) * torch.exp(-a * a)
    y = 0.5 * z * (1 + erf)
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    dgelu = 0.5 * (1 + erf) + z * phi
    bound = 0.5 * z.abs() * (2 * ERF_ULP * U32 * erf.abs() + derf * 2 * U32 * a.abs() + U32 * (1 + erf).abs()) + U32 * y.abs() + dgelu.abs() * dz + FLT_MIN
    return y, bound


def worst(got, ref, bound):
    """max |got - ref| / bound (an exact match counts 0 whatever its bound, a non-finite value inf)"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    diff = (got - ref).abs()
    r = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return r.max().item()
