"""CPU checks of the layer-aggregator restatement (tests/agg_ref.py): known answers, float64 gradcheck, the packed layout
against the dense one, and the committed fixtures against a fresh run of their generator."""
import os
import sys

import numpy as np
import pytest
import torch

import agg_ref as AR
from bmp import packed, synth

T_ = torch.from_numpy


def _hs(T, shape=(3, 5, 4), seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, dtype=torch.float64, generator=g) for _ in range(T)]


def test_single_layer_is_the_identity():
    (h,) = _hs(1)
    W, b = torch.tensor([[0.7]], dtype=torch.float64), torch.tensor([-0.2], dtype=torch.float64)
    assert torch.equal(AR.layer_aggregate([h], "max-pool"), h)
    assert torch.allclose(AR.layer_aggregate([h], "attn", W, b), h, rtol=0, atol=1e-15)
    assert torch.equal(AR.layer_aggregate([h], "concat"), h)


def test_zero_attention_weights_give_the_mean_over_layers():
    hs = _hs(4)
    y = AR.layer_aggregate(hs, "attn", torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    assert torch.allclose(y, torch.stack(hs).mean(dim=0), rtol=0, atol=1e-14)


@pytest.mark.parametrize("s", [0, 2])
def test_large_bias_selects_a_layer(s):
    hs = _hs(3)
    g = torch.Generator().manual_seed(1)
    W = 0.1 * torch.randn(3, 3, dtype=torch.float64, generator=g)
    b = torch.zeros(3, dtype=torch.float64)
    b[s] = 200.0
    assert torch.allclose(AR.layer_aggregate(hs, "attn", W, b), hs[s], rtol=0, atol=1e-12)


def test_attention_acts_on_the_layer_axis_per_channel():
    """One element written out: z_s = sum_t W[s, t] x_t + b_s, y = sum_s softmax(z)_s x_s."""
    hs = _hs(3, shape=(2, 2, 2), seed=3)
    g = torch.Generator().manual_seed(4)
    W, b = torch.randn(3, 3, dtype=torch.float64, generator=g), torch.randn(3, dtype=torch.float64, generator=g)
    y = AR.layer_aggregate(hs, "attn", W, b)
    x = torch.stack([h[1, 0, 1] for h in hs])
    p = torch.softmax(W @ x + b, dim=0)
    assert abs(float(y[1, 0, 1]) - float((p * x).sum())) < 1e-14


def test_max_gradient_goes_to_every_tied_position():
    a = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([1.0, 5.0, 3.0], dtype=torch.float64, requires_grad=True)
    AR.layer_aggregate([a, b], "max-pool").backward(torch.tensor([10.0, 20.0, 30.0], dtype=torch.float64))
    assert a.grad.tolist() == [10.0, 0.0, 30.0] and b.grad.tolist() == [10.0, 20.0, 30.0]


@pytest.mark.parametrize("agg", AR.AGGREGATORS)
def test_gradcheck(agg):
    hs = [h.requires_grad_() for h in _hs(3, shape=(2, 3, 4), seed=5)]
    g = torch.Generator().manual_seed(6)
    W = torch.randn(3, 3, dtype=torch.float64, generator=g).requires_grad_()
    b = torch.randn(3, dtype=torch.float64, generator=g).requires_grad_()
    if agg == "attn":
        assert torch.autograd.gradcheck(lambda W, b, *h: AR.layer_aggregate(h, agg, W, b), (W, b, *hs))
    else:
        assert torch.autograd.gradcheck(lambda *h: AR.layer_aggregate(h, agg), tuple(hs))


@pytest.mark.parametrize("agg", AR.AGGREGATORS)
@pytest.mark.parametrize("tied", [True, False])
def test_packed_form_equals_dense_form(agg, tied):
    """The virtual pad row (one row, multiplicity row_w) against the dense batch with all its padded positions."""
    store = synth.make_store(9, seed=11, n_lo=2, n_hi=14, n_mean=6)
    store.append(synth.Molecule(np.array([6, 8, 7, 6], np.int32), np.array([[0, 1, 0], [1, 2, 1]], np.int32)))
    atoms, adj = synth.concat_mols(store)
    pb = packed.pack_from_dense([atoms], [adj])
    assert float(pb.row_w.max()) > 1.0                      # some molecule is padded by more than one position
    p = AR.make_agg_params(3, 16, 8, 3, agg, weight_tying=tied)
    g, _ = AR.ggnn_agg_forward(p, T_(atoms), T_(adj).double(), 3, agg, weight_tying=tied)
    gp, _ = AR.ggnn_agg_forward_packed(p, pb, 3, agg, weight_tying=tied)
    assert float((g - gp).abs().max()) <= 1e-12 * float(g.abs().max())


@pytest.mark.parametrize("agg", AR.AGGREGATORS)
def test_fixture_equals_fresh_generator_run(agg, golden_dir):
    sys.path.insert(0, golden_dir)
    try:
        import make_golden_agg as M
    finally:
        sys.path.remove(golden_dir)
    fresh = M.build(agg)
    with np.load(os.path.join(golden_dir, M.FILES[agg])) as z:
        assert sorted(z.files) == sorted(fresh)
        for k in z.files:
            a, b = z[k], fresh[k]
            assert a.shape == b.shape and a.dtype == b.dtype, k
            scale = max(float(np.abs(b).max()), 1e-30)
            assert float(np.abs(a.astype(np.float64) - b).max()) <= 1e-6 * scale, k
        if agg == "max-pool":
            assert min(float(z[k]) for k in z.files if k.endswith(":gap")) >= M.MAX_GAP
        assert atoms_have_padding_and_an_isolated_atom(z["atoms"], z["adj"])


def atoms_have_padding_and_an_isolated_atom(atoms, adj):
    n = (atoms != 0).sum(axis=1)
    deg = adj.sum(axis=(1, 3))
    return len(set(n.tolist())) > 2 and bool(((atoms != 0) & (deg == 0)).any())
