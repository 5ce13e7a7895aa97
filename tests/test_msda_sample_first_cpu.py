"""Host side of the sample-first MSDeformAttn path: the size rule and the switch (ops/modules/ms_deform_attn.py)."""
import glob
import json
import os

import numpy as np
import pytest

from ocpg_amd.models.ops.modules import ms_deform_attn as mda

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture_sizes():
    """(name, N, S, M, Lq, L, P) of every committed fixture that describes level shapes: the cross-attention call a model of that size makes"""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        z = np.load(path)
        if "__meta__" not in z.files:
            continue
        m = json.loads(bytes(z["__meta__"]).decode())
        cfg = m.get("cfg", {}) if isinstance(m.get("cfg"), dict) else {}
        shapes = m.get("shapes")
        if not shapes or not all(isinstance(s, (list, tuple)) and len(s) == 2 for s in shapes):
            continue
        S = sum(int(h) * int(w) for h, w in shapes)
        N = int(m.get("N", m.get("B", 1) * m.get("T", 1)))
        M = int(m.get("M", m.get("nhead", cfg.get("nheads", 8))))
        Lq = int(m.get("Lq", m.get("Q", cfg.get("num_queries", 5))))
        out.append((os.path.basename(path), N, S, M, Lq, len(shapes), int(m.get("P", 4))))
    return out


def test_rule_is_false_at_every_fixture_size():
    sizes = _fixture_sizes()
    assert any(n.startswith("msda_module") for n, *_ in sizes) and any(n.startswith("transformer") for n, *_ in sizes), sizes
    for name, N, S, M, Lq, L, P in sizes:
        assert not mda.sample_first_wanted(N, S, M, Lq, L, P), name
        assert not mda.sample_first_wanted(N, S, M, S, L, P), name


@pytest.mark.parametrize("N,S,M,Lq,L,P", [(10, 5100, 8, 5, 4, 4), (5, 5100, 8, 5, 4, 4), (8, 8100, 8, 5, 4, 4)])
def test_rule_is_true_at_model_sizes(N, S, M, Lq, L, P):
    assert mda.sample_first_wanted(N, S, M, Lq, L, P)
    assert not mda.sample_first_wanted(N, S, M, S, L, P)          # self-attention: every value is read
    assert not mda.sample_first_wanted(N, S, M, S // 2, L, P)     # too many queries for the gather to stay small


def test_rule_needs_a_large_value_projection():
    from ocpg_amd.models import amp_cache
    rows = amp_cache.TOKEN_LINEAR_MIN_ROWS
    assert not mda.sample_first_wanted(1, rows - 1, 8, 5, 4, 4)
    assert mda.sample_first_wanted(1, rows, 8, 5, 4, 4)


def test_switch_words():
    assert [mda.sample_first_mode(w) for w in ("0", "1", "force")] == ["0", "1", "force"]
    for bad in ("", "2", "on", "Force"):
        with pytest.raises(ValueError):
            mda.sample_first_mode(bad)
    assert mda.SAMPLE_FIRST in ("0", "1", "force")
