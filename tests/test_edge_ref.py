"""Known answers that pin the float64 restatement of the GGNN with message_function='edge_network' (tests/edge_ref.py) to the
reference's EdgeNetwork (models/ggnn.py:657-720): the golden vectors (made by the plain-numpy transcription in
tests/golden/make_golden_edge.py), the closed form against the op-for-op form, and identities that need no oracle.  No GPU."""
import os

import numpy as np
import pytest
import torch

import edge_ref as R
from bmp import synth

D, OUT = 8, 4


def _batch():
    return synth.concat_mols(synth.make_store(4, seed=3, n_lo=2, n_hi=9, n_mean=5))


def _more_positions(atoms, adj, k):
    mb, A = atoms.shape
    a = np.zeros((mb, A + k), np.int32); a[:, :A] = atoms
    j = np.zeros((mb, 4, A + k, A + k), np.float32); j[:, :, :A, :A] = adj
    return a, j


def test_golden_vectors():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ggnn_edge_small.npz"))
    atoms, adj = z["atoms"], z["adj"]
    assert atoms.shape[0] == 3 and (atoms == 0).any()                   # the batch is padded
    for tag, cfg in (("tied", dict(layers=3, tying=True, concat_hidden=False)), ("untied", dict(layers=3, tying=False, concat_hidden=True))):
        pre = tag + ":p:"
        p = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
        assert sorted(p) == sorted(R.make_params(0, D, OUT, cfg["layers"], cfg["tying"], cfg["concat_hidden"]))
        for message in (R.edge_message_dense, R.edge_message_closed):
            g, hs = R.forward(p, atoms, adj, message=message, **cfg)
            assert g.shape == (3, (3 if cfg["concat_hidden"] else 1) * OUT)
            assert np.abs(g.numpy() - z[tag + ":g"]).max() < 1e-12
            assert np.abs(torch.stack(hs).numpy() - z[tag + ":hs"]).max() < 1e-12


@pytest.mark.parametrize("name", R.DATA_SETS)
def test_closed_form_is_the_dense_network(name):
    """m = sum_e W_e . agg_e + B . S against EdgeNetwork.__call__ op for op, float64, on every data set (real rows and pad
    positions alike) and for adjacency VALUES other than 0 / 1: the network is affine in them."""
    gen = torch.Generator().manual_seed(3)
    for atoms, adj in R.data(name)["sides"]:
        mb, A = atoms.shape
        h = torch.randn(mb, A, D, dtype=torch.float64, generator=gen)
        W = torch.randn(D * D, 4, dtype=torch.float64, generator=gen) * 0.3
        b = torch.randn(D * D, dtype=torch.float64, generator=gen) * (0.3 / max(A, 1))
        for j in (torch.as_tensor(adj).double(), torch.as_tensor(adj).double() * torch.rand(adj.shape, dtype=torch.float64, generator=gen)):
            dense, closed = R.edge_message_dense(h, j, W, b), R.edge_message_closed(h, j, W, b)
            assert dense.abs().max() > 1e-2
            assert (dense - closed).abs().max() <= 1e-12 * max(1.0, dense.abs().max().item())
    # ... and through the whole encoder, forward and gradients
    c = dict(R.CASES["edge16"], data=name)
    atoms, adj = R.data(name)["sides"][0]
    res = []
    for message in (R.edge_message_dense, R.edge_message_closed):
        p = {k: v.requires_grad_() for k, v in R.case_params(c).items()}
        g, hs = R.forward(p, atoms, adj, c["layers"], c["tying"], message=message)
        (g.sum() + hs[-1].sum()).backward()
        res.append((g.detach(), hs[-1].detach(), {k: v.grad for k, v in p.items()}))
    assert (res[0][0] - res[1][0]).abs().max() < 1e-12 and (res[0][1] - res[1][1]).abs().max() < 1e-12
    for k, gr in res[0][2].items():
        if gr is None:
            assert res[1][2][k] is None and "hidden_layers" in k            # built and never called
        else:
            assert (gr - res[1][2][k]).abs().max() <= 1e-12 * max(1.0, gr.abs().max().item()), k


def test_atom_states_depend_on_the_padded_atom_count():
    """The same molecules padded to A and to A + 3: the REAL atoms' states differ (S counts every padded position), which no
    other encoder here does -- the reason the encoder layout and dedup are refused; a molecule's pad positions share one state."""
    atoms, adj = _batch()
    a3, j3 = _more_positions(atoms, adj, 3)
    p = R.make_params(5, D, OUT, 3, True, a_typ=atoms.shape[1])
    _, hs = R.forward(p, atoms, adj, 3)
    _, hs3 = R.forward(p, a3, j3, 3)
    A = atoms.shape[1]
    real = torch.as_tensor(atoms != 0)
    assert (hs3[-1][:, :A][real] - hs[-1][real]).abs().max() > 1e-3
    pad = hs3[-1][:, A:]                                                 # three appended positions per molecule
    assert (pad - pad[:, :1]).abs().max() == 0
    for b in range(atoms.shape[0]):                                      # ... equal to the molecule's earlier pad positions, if any
        n = int((atoms[b] != 0).sum())
        if n < A:
            assert (hs3[-1][b, n:A] - hs3[-1][b, A]).abs().max() < 1e-14


def test_zero_bias_is_the_matrix_multiply_message():
    """B = 0 and W_e taken from a matrix_multiply model whose message bias is zero: the two restatements agree (the typed
    neighbour sums are the same arithmetic)."""
    atoms, adj = _batch()
    for tying, concat in ((True, False), (False, True)):
        p = R.make_params(3, D, OUT, 3, tying, concat)
        q = {k: v for k, v in p.items() if "message_layers" not in k}
        gen = torch.Generator().manual_seed(9)
        for i in range(1 if tying else 3):
            Wm = torch.randn(4 * D, D, dtype=torch.float64, generator=gen) * 0.2          # GraphLinear(d, 4d): row 4 c + e
            q[f"message_layers/{i}/W"], q[f"message_layers/{i}/b"] = Wm, torch.zeros(4 * D, dtype=torch.float64)
            # W_e[p, k] = Wm[4 p + e, k]  ->  output_layer.W[p d + k, e]
            p[f"message_layers/{i}/output_layer/W"] = Wm.reshape(D, 4, D).permute(0, 2, 1).reshape(D * D, 4)
            p[f"message_layers/{i}/output_layer/b"] = torch.zeros(D * D, dtype=torch.float64)
        g, hs = R.forward(p, atoms, adj, 3, tying, concat)
        go, ho = R.O.ggnn_forward(q, torch.as_tensor(atoms), torch.as_tensor(adj).double(), 3, tying, concat)
        assert (g - go).abs().max() < 1e-12 and (hs[-1] - ho).abs().max() < 1e-12
        # ... and a bias that is not zero moves it
        p["message_layers/0/output_layer/b"] = torch.full((D * D,), 0.05, dtype=torch.float64)
        assert (R.forward(p, atoms, adj, 3, tying, concat)[0] - go).abs().max() > 1e-2


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_update_gates_are_not_saturated(name):
    """A saturated GRU would hide a wrong message: every case keeps at least half of its last step's update-gate values
    inside (0.05, 0.95) in float64."""
    assert R.gate_share(R.CASES[name]) >= 0.5


def test_unread_parameters_and_edge_hidden_dim_do_not_matter():
    atoms, adj = _batch()
    p = R.make_params(7, D, OUT, 2, True)
    q = {k: (v if "hidden_layers" not in k else v + 1.0) for k, v in p.items()}
    assert torch.equal(R.forward(p, atoms, adj, 2)[0], R.forward(q, atoms, adj, 2)[0])
    r = R.make_params(7, D, OUT, 2, True, edge_hidden=5)                 # (drawn after output_layer: the draws before it agree)
    assert r["message_layers/0/hidden_layers/0/W"].shape == (5, 4)
    assert torch.equal(r["message_layers/0/output_layer/W"], p["message_layers/0/output_layer/W"])


def test_atom_permutation_invariance():
    atoms, adj = _batch()
    A = atoms.shape[1]
    perm = np.random.RandomState(0).permutation(A)
    ap, jp = atoms[:, perm], adj[:, :, perm][:, :, :, perm]
    for concat in (False, True):
        p = R.make_params(6, D, OUT, 3, False, concat)
        g, hs = R.forward(p, atoms, adj, 3, False, concat)
        gp, hsp = R.forward(p, ap, jp, 3, False, concat)
        assert torch.allclose(g, gp, atol=1e-12)
        assert torch.allclose(hs[-1][:, perm], hsp[-1], atol=1e-12)


def test_single_tile_data_sets():
    many, full = R.data("many")["pb"], R.data("full")["pb"]
    assert many.n_tiles == 1 and many.n_mols == 64 and (many.mol_nrows == 2).all() and not many.oversized
    assert full.n_tiles == 2 and int(full.mol_nrows.max()) == 128 and not full.oversized
