"""Reference composition of the mask head's memory fusion: the torch lines csrc/mask_front.hip stands for (models/deformable_transformer.py:
the NCHW copies of the memory's levels; models/ocpg.py: sum(bicubic_resize(x.float(), tar)); decoder._nhwc: the channels-last copy), written
so that they run in any dtype on any device: fp64 on the CPU is the reference, fp32 on the GPU is what the step ran before the kernel."""
import torch

from ocpg_amd.models.resample import bicubic_matrix

EPS32 = 2.0 ** -24      # unit roundoff of fp32

GEOMETRIES = {
    "odd": ((7, 9), (4, 5), (2, 3)),                    # odd and non-dividing
    "even": ((8, 12), (4, 6), (2, 3)),
    "four": ((7, 9), (4, 5), (2, 3), (1, 2)),           # a 4-level memory of which 3 are read
    "tiny_model": ((24, 28), (12, 14), (6, 7), (3, 4)),  # the model-level test's step: several row tiles per level, ranges of 8 and 16 rows
}


def level_maps(memory, shapes, n_lvl):
    nb, _, c = memory.shape
    feats, start = [], 0
    for (h, w) in shapes[:n_lvl]:
        feats.append(memory[:, start:start + h * w].reshape(nb, h, w, c).permute(0, 3, 1, 2).contiguous())
        start += h * w
    return feats


def resize(x, size, absw=False):
    h, w = x.shape[-2:]
    H, W = size
    if (h, w) == (H, W):
        return x
    wy = bicubic_matrix(h, H, x.device).to(x.dtype)
    wx = bicubic_matrix(w, W, x.device).to(x.dtype)
    if absw:
        wy, wx = wy.abs(), wx.abs()
    return torch.matmul(wy, torch.matmul(x, wx.t()))


def compose(memory, shapes, n_lvl, absw=False):
    """-> (fusion NCHW, the same channels-last).  absw: the matrices' absolute values (with |memory| this gives, per element, the sum of
    the magnitudes of the terms: the scale of a rounding error of that element)."""
    feats = level_maps(memory, shapes, n_lvl)
    tar = feats[0].shape[-2:]
    fusion = sum(resize(x, tar, absw) for x in feats)
    return fusion, fusion.permute(0, 2, 3, 1).contiguous()


def compose_with_grad(memory, shapes, n_lvl, g_nchw, g_cl, absw=False):
    """-> (fusion NCHW, gradient of memory for the port gradients given; a None gradient leaves that port out)."""
    m = memory.detach().clone().requires_grad_(True)
    nchw, cl = compose(m, shapes, n_lvl, absw)
    outs, gs = [], []
    if g_nchw is not None:
        outs.append(nchw), gs.append(g_nchw)
    if g_cl is not None:
        outs.append(cl), gs.append(g_cl)
    (gm,) = torch.autograd.grad(outs, [m], gs)
    return nchw.detach(), gm


def reference(memory, shapes, n_lvl, g_nchw, g_cl):
    """fp64 on the CPU: (fusion, gradient, scale of the fusion's rounding error, scale of the gradient's): the scales are EPS32 times the
    sums of the terms' magnitudes."""
    d = lambda t: None if t is None else t.detach().double().cpu()
    m, gn, gc = d(memory), d(g_nchw), d(g_cl)
    out, gm = compose_with_grad(m, shapes, n_lvl, gn, gc)
    out_mag, gm_mag = compose_with_grad(m.abs(), shapes, n_lvl, None if gn is None else gn.abs(), None if gc is None else gc.abs(), absw=True)
    return out, gm, EPS32 * out_mag, EPS32 * gm_mag


def distance(got, ref, scale):
    """max over the elements of |got - ref| in units of the element's own rounding scale (elements whose scale is 0 must be equal)."""
    err = (got.detach().double().cpu() - ref).abs()
    zero = scale == 0
    assert bool((err[zero] == 0).all())
    return float((err[~zero] / scale[~zero]).max()) if bool((~zero).any()) else 0.0


# ---- level-set feature stack ------------------------------------------------------------------------------------------------------
from ocpg_amd.models.resample import bilinear_matrix  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def bilinear(x, size):
    """resample.bilinear_resize(x, size, align_corners=True) in x's own dtype (the product's version always computes in fp32)."""
    wy = bilinear_matrix(x.shape[-2], size[0], True, x.device).to(x.dtype)
    wx = bilinear_matrix(x.shape[-1], size[1], True, x.device).to(x.dtype)
    return torch.matmul(wy, torch.matmul(x, wx.t()))


def ls_compose(lsf, txt8, frames, b, t):
    """Today's lines of ocpg.py: lsf [b*t, 8, h, w], txt8 [b, 8], frames [b*t, 3, H, W] -> ls_features [b, t, 12, 4h, 4w]."""
    ls_feat = bilinear(lsf, (4 * lsf.shape[-2], 4 * lsf.shape[-1])).unflatten(0, (b, t))
    txt = txt8[:, None, :, None, None]
    sim = (ls_feat * txt).sum(dim=2) / ((F.normalize(ls_feat, dim=2) * F.normalize(txt, dim=2)).sum(dim=2) + 1e-5)
    img = bilinear(frames, tuple(ls_feat.shape[-2:])).unflatten(0, (b, t))
    return torch.cat([img, ls_feat, sim.unsqueeze(2)], dim=2)


def ls_compose_with_grad(lsf, txt8, frames, b, t, g):
    l, x = lsf.detach().clone().requires_grad_(True), txt8.detach().clone().requires_grad_(True)
    out = ls_compose(l, x, frames, b, t)
    gl, gt = torch.autograd.grad([out], [l, x], [g], allow_unused=True)
    return out.detach(), gl, (torch.zeros_like(x) if gt is None else gt)


def ls_reference(lsf, txt8, frames, b, t, g):
    """fp64 on the CPU: outputs, gradients, the per-element rounding scale of the output, and |den| of sim.
    Scale: channels 0-10 are sums of non-negative weights times values: EPS32 * the same interpolation of |values|; channel 11 is
    dot / den: EPS32 * (sum_c |f_c t_c| / |den| + |dot| / den^2), the first-order effect of one rounding in dot and one in den (|cos|
    terms sum to at most 1)."""
    d = lambda v: v.detach().double().cpu()
    l, x, fr, gg = d(lsf), d(txt8), d(frames), d(g)
    out, gl, gt = ls_compose_with_grad(l, x, fr, b, t, gg)
    mag = ls_compose(l.abs(), x.abs(), fr.abs(), b, t)
    f = out[:, :, 3:11]
    tv = x[:, None, :, None, None]
    dot = (f * tv).sum(2)
    den = (F.normalize(f, dim=2) * F.normalize(tv, dim=2)).sum(2) + 1e-5
    scale = EPS32 * mag
    scale[:, :, 11] = EPS32 * ((f * tv).abs().sum(2) / den.abs() + dot.abs() / den ** 2)
    return out, gl, gt, scale, den.abs()


def grad_scale(ref):
    """Scale of a gradient tensor's rounding error: EPS32 * (|element| + the tensor's mean magnitude) -- the elements are sums of terms of
    the tensor's typical size, which may cancel."""
    return EPS32 * (ref.abs() + ref.abs().mean())
