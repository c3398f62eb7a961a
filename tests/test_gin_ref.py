"""Known answers that pin the float64 GIN restatement (tests/gin_ref.py) to the description of the reference's models/gin.py,
and the relu kink condition of every row of its table of test cases.  No GPU, no oracle."""
import os

import numpy as np
import pytest
import torch

import gin_ref as GR
from bmp import synth

D, O = 8, 5


def _U(p, i, k):
    return p[f"update_layers/{i}/linear_g{k}/W"], p[f"update_layers/{i}/linear_g{k}/b"]


def test_zero_bond_molecule_has_s_equal_h():
    p = GR.make_gin_params(1, D, O, 1, True)
    atoms = np.array([[6, 8, 7]], np.int32)
    adj = np.zeros((1, 4, 3, 3), np.float32)
    _, h = GR.gin_forward(p, atoms, adj)
    (W1, b1), (W2, b2) = _U(p, 0, 1), _U(p, 0, 2)
    e = p["embed/W"][torch.tensor([6, 8, 7])]
    want = torch.relu(torch.relu(e @ W1.t() + b1) @ W2.t() + b2)
    assert torch.allclose(h[0], want, atol=1e-14)


def test_tied_four_layers_equal_one_layer():
    store = synth.make_store(4, seed=3, n_lo=2, n_hi=9, n_mean=5)
    atoms, adj = synth.concat_mols(store)
    p4, p1 = GR.make_gin_params(2, D, O, 4, True), GR.make_gin_params(2, D, O, 1, True)
    assert sorted(p4) == sorted(p1)
    g4, h4 = GR.gin_forward(p4, atoms, adj, tying=True)
    g1, h1 = GR.gin_forward(p1, atoms, adj, tying=True)
    assert torch.equal(g4, g1) and torch.equal(h4, h1)
    # concat_hidden: four readout layers exist, one is used; the width is ONE out_dim
    pc = GR.make_gin_params(2, D, O, 4, True, concat_hidden=True)
    assert sum(k.endswith("i_layer/W") for k in pc) == 4
    gc, _ = GR.gin_forward(pc, atoms, adj, tying=True, concat_hidden=True)
    assert gc.shape == (4, O) and torch.equal(gc, g1)
    # untied: every layer runs and concat_hidden is n_layers wide
    pu = GR.make_gin_params(2, D, O, 3, False, concat_hidden=True)
    gu, _ = GR.gin_forward(pu, atoms, adj, tying=False, concat_hidden=True)
    assert gu.shape == (4, 3 * O)


def test_padding_affine_law():
    """g(A + 1) - g(A) is one vector for every molecule: a padded position has no neighbours and reads no other position."""
    p = GR.make_gin_params(4, D, O, 3, False)
    store = synth.make_store(5, seed=3, n_lo=2, n_hi=9, n_mean=5)
    atoms, adj = synth.concat_mols(store)
    mb, A = atoms.shape
    gs = []
    for extra in (0, 1, 2):
        a = np.zeros((mb, A + extra), np.int32); a[:, :A] = atoms
        j = np.zeros((mb, 4, A + extra, A + extra), np.float32); j[:, :, :A, :A] = adj
        gs.append(GR.gin_forward(p, a, j, tying=False)[0])
    step = gs[1] - gs[0]
    assert torch.allclose(step, step[0].expand_as(step), atol=1e-12) and step.abs().max() > 1e-3
    assert torch.allclose(gs[2] - gs[1], step, atol=1e-12)


def test_atom_permutation_invariance():
    p = GR.make_gin_params(5, D, O, 2, False, concat_hidden=True)
    store = synth.make_store(3, seed=8, n_lo=4, n_hi=10, n_mean=7)
    atoms, adj = synth.concat_mols(store)
    g, _ = GR.gin_forward(p, atoms, adj, tying=False, concat_hidden=True)
    perm = np.random.RandomState(0).permutation(atoms.shape[1])
    g2, _ = GR.gin_forward(p, atoms[:, perm], adj[:, :, perm][:, :, :, perm], tying=False, concat_hidden=True)
    assert torch.allclose(g, g2, atol=1e-12)


def test_bond_type_does_not_matter_and_values_count():
    p = GR.make_gin_params(6, D, O, 2, False)
    store = synth.make_store(3, seed=8, n_lo=4, n_hi=10, n_mean=7)
    atoms, adj = synth.concat_mols(store)
    g, h = GR.gin_forward(p, atoms, adj, tying=False)
    g2, h2 = GR.gin_forward(p, atoms, np.roll(adj, 1, axis=1), tying=False)
    one = np.zeros_like(adj); one[:, 2] = adj.sum(axis=1)
    g3, h3 = GR.gin_forward(p, atoms, one, tying=False)
    assert torch.allclose(g, g2, atol=1e-13) and torch.allclose(h, h3, atol=1e-13) and torch.allclose(g, g3, atol=1e-13)
    _, h4 = GR.gin_forward(p, atoms, 2 * adj, tying=False)             # an entry counts with its value
    assert not torch.allclose(h, h4, atol=1e-3)


def test_keep_mask_sits_between_the_second_linear_and_its_relu():
    p = GR.make_gin_params(7, D, O, 1, True)
    atoms, adj = synth.concat_mols(synth.make_store(2, seed=5, n_lo=3, n_hi=6, n_mean=4))
    keep = (torch.rand(atoms.shape + (D,), generator=torch.Generator().manual_seed(1)) >= 0.5).double() * 2.0
    _, h = GR.gin_forward(p, atoms, adj, keep=[keep])
    _, hn = GR.gin_forward(p, atoms, adj)
    assert torch.allclose(h, 2.0 * hn * (keep != 0), atol=1e-14)       # relu(2 x) = 2 relu(x); a zeroed element gives relu(0) = 0


def test_is_real_node_masks_the_readout_sum():
    p = GR.make_gin_params(8, D, O, 1, True)
    atoms, adj = synth.concat_mols(synth.make_store(3, seed=5, n_lo=2, n_hi=6, n_mean=4))
    real = (atoms != 0).astype(np.float32)
    g, _ = GR.gin_forward(p, atoms, adj, is_real_node=real)
    for b in range(3):
        n = int(real[b].sum())
        gb, _ = GR.gin_forward(p, atoms[b:b + 1, :n], adj[b:b + 1, :, :n, :n])
        assert torch.allclose(g[b], gb[0], atol=1e-13)


def test_golden_vectors():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gin_small.npz"))
    p = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p:")}
    assert z["two:atoms"].shape == (1, 2) and z["ring:atoms"].shape == (1, 5) and z["batch:atoms"].shape[0] == 3
    assert (z["batch:atoms"] == 0).any()                               # the batch is padded
    for name in ("two", "ring", "batch"):
        g, h = GR.gin_forward(p, z[name + ":atoms"], z[name + ":adj"], tying=False, concat_hidden=True)
        assert np.abs(g.numpy() - z[name + ":g"]).max() < 1e-12 and np.abs(h.numpy() - z[name + ":h"]).max() < 1e-12


@pytest.mark.parametrize("name", sorted(GR.KINK_TABLE))
def test_kink_condition_of_every_table_row(name):
    lo, err = GR.kink_margin(GR.KINK_TABLE[name])
    print(f"[kink] {name}: min |pre64| {lo:.3e}, max |pre32 - pre64| {err:.3e}, margin {lo / err:.1f} x")
    assert err > 0 and lo >= GR.KINK_FACTOR * err
