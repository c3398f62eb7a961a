"""CPU checks of the layer-aggregator plumbing: the constructor's parameters and refusals, the missing atom array, the
plan protocol's tables, and the new entry points in the header, the ctypes table and the gfx950-only library."""
import os
import re

import pytest
import torch

from bmp.ggnn import GGNN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bmp_layer_agg_ws_floats", "bmp_layer_agg_fwd", "bmp_layer_agg_bwd")


def _shapes(m):
    return {n: tuple(p.shape) for n, p in m.named_parameters()}


@pytest.mark.parametrize("T", [3, 8])
def test_attn_parameters(T):
    m = GGNN(out_dim=8, hidden_dim=16, n_layers=T, layer_aggregator="attn", weight_tying=False)
    s = _shapes(m)
    assert s["attn_dense_layer.W"] == (T, T) and s["attn_dense_layer.b"] == (T,)
    assert float(m.attn_dense_layer.b.detach().abs().max()) == 0.0                    # Chainer's Linear: zero bias
    assert s["i_layers.0.W"] == (8, 32) and s["j_layers.0.W"] == (8, 16)
    assert not any(n.startswith(("bigru_layer", "bilstm_layer")) for n in s)
    assert m.plannable()


def test_max_pool_has_no_parameters_of_its_own():
    plain = _shapes(GGNN(out_dim=8, hidden_dim=16, n_layers=4))
    assert _shapes(GGNN(out_dim=8, hidden_dim=16, n_layers=4, layer_aggregator="max-pool")) == plain


def test_concat_sizes_the_readout_layers():
    T, d = 4, 16
    m = GGNN(out_dim=8, hidden_dim=d, n_layers=T, layer_aggregator="concat")
    s = _shapes(m)
    assert s["i_layers.0.W"] == (8, 2 * T * d) and s["j_layers.0.W"] == (8, T * d)
    assert "attn_dense_layer.W" not in s and not m.plannable()


def test_concat_hidden_keeps_its_readout_layers_as_parameters():
    m = GGNN(out_dim=8, hidden_dim=16, n_layers=3, layer_aggregator="max-pool", concat_hidden=True)
    assert len(m.i_layers) == 3 and len(m.j_layers) == 3


@pytest.mark.parametrize("name", ["gru", "lstm", "gru-attn", "lstm-attn", "self-attn"])
def test_recurrent_aggregators_are_refused_with_the_reason(name):
    with pytest.raises(NotImplementedError, match="NStepBiGRU"):
        GGNN(out_dim=8, hidden_dim=16, layer_aggregator=name)


def test_unknown_aggregator_is_a_value_error():
    with pytest.raises(ValueError, match="layer aggregator"):
        GGNN(out_dim=8, hidden_dim=16, layer_aggregator="mean")


@pytest.mark.parametrize("agg", ["attn", "max-pool"])
def test_more_than_eight_layers_is_a_value_error(agg):
    with pytest.raises(ValueError, match="n_layers"):
        GGNN(out_dim=8, hidden_dim=16, n_layers=9, layer_aggregator=agg)
    GGNN(out_dim=8, hidden_dim=16, n_layers=9, layer_aggregator="concat")


def test_operator_refuses_nine_tensors_before_any_launch():
    from bmp import functional as Fn
    hs = [torch.zeros(128, 16) for _ in range(9)]           # host tensors: the count is checked first
    with pytest.raises(ValueError, match="n_layers"):
        Fn.LayerAggFn.apply(0, None, None, *hs)


@pytest.mark.parametrize("agg", ["concat", "max-pool", "attn"])
def test_get_atom_array_fails_clearly(agg):
    m = GGNN(out_dim=8, hidden_dim=16, n_layers=3, layer_aggregator=agg)
    with pytest.raises(RuntimeError, match="layer_aggregator"):
        m.get_atom_array()


def test_plan_tables_carry_the_attention_layer():
    from bmp.plan import LayoutPlan
    m = GGNN(out_dim=8, hidden_dim=16, n_layers=3, layer_aggregator="attn", weight_tying=False)
    names, shapes = [n for n, _ in m.named_parameters()], [tuple(p.shape) for _, p in m.named_parameters()]
    plan = LayoutPlan([("", m)], names, shapes, "cpu")
    assert plan.prep_slices[""]["agg.W"][1] == (3, 3) and plan.prep_slices[""]["agg.b"][1] == (3,)
    assert plan.gk_slices[""]["agg.dW"][1] == (3, 3) and plan.gk_slices[""]["agg.db"][1] == (3,)
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    plan.prepare(flat)
    assert torch.equal(plan.P[""]["agg.W"], m.attn_dense_layer.W.detach())
    plan.gk.copy_(torch.arange(plan.n_gk, dtype=torch.float32))
    g = torch.zeros_like(flat)
    plan.collect(g)
    off = sum(int(torch.tensor(s).prod()) for n, s in zip(names, shapes) if names.index(n) < names.index("attn_dense_layer.W"))
    assert torch.equal(g[off:off + 9].view(3, 3), plan.G[""]["agg.dW"])
    pm = GGNN(out_dim=8, hidden_dim=16, n_layers=3, layer_aggregator="max-pool")
    pplan = LayoutPlan([("", pm)], [n for n, _ in pm.named_parameters()], [tuple(p.shape) for _, p in pm.named_parameters()], "cpu")
    assert not any(k.startswith("agg.") for k in pplan.prep_slices[""])


def test_header_and_ctypes_table_declare_the_entry_points():
    from bmp import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmp.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, f"{name} is not declared in include/bmp.h"
        assert name in _lib.SIGNATURES
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SIGNATURES[name][1]), name


def test_library_exports_them_and_is_gfx950_only():
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name)
    assert L.bmp_layer_agg_ws_floats(128, 16, 9) > 0 and L.bmp_layer_agg_ws_floats(1 << 20, 128, 8) == 1024 * 72
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx90a", b"gfx942", b"sm_"):
        assert other not in blob


def test_entry_points_check_their_arguments_without_a_launch():
    """T > 8 and a width that is no multiple of 4 come back as argument-check codes (< -1000), before any GPU call."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    arr = (ctypes.c_void_p * 9)(*[ctypes.addressof(buf)] * 9)
    y = ctypes.addressof(buf)
    assert L.bmp_layer_agg_fwd(arr, 9, 128, 16, 0, None, None, y, None, None) < -1000
    assert L.bmp_layer_agg_fwd(arr, 4, 128, 18, 0, None, None, y, None, None) < -1000
    assert L.bmp_layer_agg_fwd(arr, 4, 128, 16, 1, None, None, y, None, None) < -1000          # attn without W
    assert L.bmp_layer_agg_bwd(y, arr, 9, 128, 16, 1, y, None, None, arr, y, None, 0, y, 1 << 20, None) < -1000
    with pytest.raises(ValueError):
        _lib.check(L.bmp_layer_agg_fwd(arr, 9, 128, 16, 0, None, None, y, None, None), "bmp_layer_agg_fwd")
