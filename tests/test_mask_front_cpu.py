"""Host side of the mask-head front end (no GPU): the reference composition against F.interpolate, the tap-range tables the kernels
walk, and the lazy level maps the transformer hands to the model."""
import pytest
import torch
import torch.nn.functional as F

import mask_front_ref as ref
from ocpg_amd.models.ops.functions import mask_front_func as mf
from ocpg_amd.models.resample import bicubic_matrix


@pytest.mark.parametrize("geo", sorted(ref.GEOMETRIES))
def test_reference_composition_is_bicubic_interpolation(geo):
    """The lines the kernel stands for, in fp64, against PyTorch's own bicubic (the matrices are built in fp32: 1e-6)."""
    shapes = ref.GEOMETRIES[geo]
    torch.manual_seed(0)
    memory = torch.randn(2, sum(h * w for h, w in shapes), 8, dtype=torch.float64)
    nchw, cl = ref.compose(memory, shapes, 3)
    feats = ref.level_maps(memory, shapes, 3)
    exp = feats[0] + sum(F.interpolate(x, size=shapes[0], mode="bicubic", align_corners=False) for x in feats[1:])
    assert torch.allclose(nchw, exp, rtol=0, atol=1e-5)
    assert torch.equal(cl, nchw.permute(0, 2, 3, 1))


@pytest.mark.parametrize("geo", sorted(ref.GEOMETRIES) + ["bench", "config5"])
def test_tables_cover_every_nonzero_entry(geo):
    """Every matrix entry that is not zero lies inside the forward range of its row and the backward range of its column; every range is
    inside its axis; the directory's offsets address exactly the tables."""
    shapes = {"bench": ((48, 80), (24, 40), (12, 20), (6, 10)), "config5": ((60, 107), (30, 54), (15, 27), (8, 14))}.get(geo) or ref.GEOMETRIES[geo]
    n_lvl = 3
    wts, rng, geom = mf.tables(shapes, n_lvl, "cpu")
    assert geom.dtype == torch.int64 and geom.shape == (len(shapes), 9)
    (h0, w0), start = shapes[0], 0
    for l, (h, w) in enumerate(shapes):
        row = geom[l].tolist()
        assert row[:3] == [h, w, start]
        start += h * w
        if not 1 <= l < n_lvl:
            assert row[3:] == [0] * 6
            continue
        for n_in, n_out, wo, fo, bo in ((h, h0, row[3], row[5], row[7]), (w, w0, row[4], row[6], row[8])):
            m = bicubic_matrix(n_in, n_out, "cpu")
            assert torch.equal(wts[wo:wo + m.numel()].view(n_out, n_in), m)          # the operands of today's matmuls, bit for bit
            f = rng[fo:fo + 2 * n_out].view(n_out, 2)
            b = rng[bo:bo + 2 * n_in].view(n_in, 2)
            for r, mat, n in ((f, m, n_in), (b, m.t(), n_out)):
                assert int(r[:, 0].min()) >= 0 and int((r[:, 0] + r[:, 1]).max()) <= n and int(r[:, 1].min()) >= 1
                idx = torch.arange(n)[None, :]
                inside = (idx >= r[:, :1]) & (idx < r[:, :1] + r[:, 1:])
                assert bool(((mat != 0) <= inside).all())
            assert int(f[:, 1].max()) <= 4                                             # four taps, clamped at the border


def test_level_maps_are_the_copies_the_transformer_made():
    shapes = ref.GEOMETRIES["four"]
    memory = torch.randn(2, sum(h * w for h, w in shapes), 8)
    lm = mf.LevelMaps(memory, shapes, 3)
    assert lm._maps is None and len(lm) == 3
    for a, b in zip(lm, ref.level_maps(memory, shapes, 3)):
        assert torch.equal(a, b) and a.is_contiguous()
    assert lm[0].shape[-2:] == shapes[0] and lm.maps() is lm.maps()


def test_op_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="CPU"):
        mf.memfuse(torch.zeros(1, 6, 4), ((2, 3),), 1)


@pytest.mark.parametrize("h,w,H,W", [(3, 5, 24, 40), (6, 10, 23, 37), (48, 80, 384, 640)])
def test_two_tap_tables_are_the_bilinear_matrices(h, w, H, W):
    """The level-set kernels' tables rebuild resample.bilinear_matrix(align_corners=True) entry for entry; the backward ranges cover every
    fine index whose tap lands on a source index."""
    from ocpg_amd.models.resample import bilinear_matrix
    Ho, Wo = 4 * h, 4 * w
    tab_i, tab_w, off = mf.ls_tables(h, w, H, W, Ho, Wo, "cpu")
    o = off.tolist()
    assert o[10] == tab_i.numel() and o[11] == tab_w.numel()
    for k, (n_in, n_out) in enumerate(((h, Ho), (w, Wo), (H, Ho), (W, Wo))):
        m = bilinear_matrix(n_in, n_out, True, "cpu")
        lo = tab_i[o[k]:o[k] + n_out].long()
        wt = tab_w[o[6 + k]:o[6 + k] + 2 * n_out].view(n_out, 2)
        back = torch.zeros(n_out, n_in)
        back.scatter_add_(1, lo[:, None], wt[:, :1])
        back.scatter_add_(1, (lo + 1).clamp(max=n_in - 1)[:, None], wt[:, 1:])
        assert torch.equal(back, m)
        if k < 2:
            r = tab_i[o[4 + k]:o[4 + k] + 2 * n_in].view(n_in, 2)
            idx = torch.arange(n_out)[None, :]
            inside = (idx >= r[:, :1]) & (idx < r[:, :1] + r[:, 1:])
            assert bool(((m.t() != 0) <= inside).all()) and int((r[:, 0] + r[:, 1]).max()) <= n_out


def test_table_cache_is_bounded():
    for n in range(mf._TABLES_MAX + 8):
        mf.ls_tables(2, 2 + n, 8, 8, 8, 4 * (2 + n), "cpu")
    assert len(mf._TABLES) <= mf._TABLES_MAX
