"""Known answers that pin the float64 NFP restatement (tests/nfp_ref.py) to the description of the reference's
models/models/nfp.py: which weight a row reads, what padding does, the degree rule and its column / row convention."""
import os

import numpy as np
import torch

import nfp_ref as NR
from bmp import synth

T = torch.from_numpy
D, O = 8, 5


def _chain(n, A):
    """A path of n atoms (ids 6) in A positions: adjacency with self loops, zero padded."""
    atoms = np.zeros((1, A), np.int32); atoms[0, :n] = 6
    adj = np.zeros((1, A, A), np.float32)
    for i in range(n):
        adj[0, i, i] = 1
        if i + 1 < n:
            adj[0, i, i + 1] = adj[0, i + 1, i] = 1
    return atoms, adj


def _B(p, l):
    return sum(p[f"layers/{l}/graph_linears/{k}/b"] for k in range(7))


def test_row_of_degree_k_reads_W_k_only():
    p = NR.make_nfp_params(1, D, O, 1)
    atoms, adj = _chain(4, 4)                                    # classes 2, 3, 3, 2 (self loop + neighbours)
    _, h = NR.nfp_forward(p, atoms, adj)
    emb = p["embed/W"][6]
    for i, (k, nb) in enumerate([(2, 2), (3, 3), (3, 3), (2, 2)]):
        want = torch.sigmoid((nb * emb) @ p[f"layers/0/graph_linears/{k - 1}/W"].t() + _B(p, 0))
        assert torch.allclose(h[0, i], want, atol=1e-14)
    q = dict(p)
    for k in (0, 3, 4, 5, 6):                                    # the other classes' weights are never read
        q[f"layers/0/graph_linears/{k}/W"] = torch.full((D, D), 1e3, dtype=torch.float64)
    _, h2 = NR.nfp_forward(q, atoms, adj)
    assert torch.equal(h, h2)


def test_padded_positions_leave_every_layer_as_sigmoid_B():
    p = NR.make_nfp_params(2, D, O, 3)
    atoms, adj = _chain(3, 6)
    for nl in (1, 2, 3):
        q = {k: v for k, v in p.items() if k == "embed/W" or int(k.split("/")[1]) < nl}
        _, h = NR.nfp_forward(q, atoms, adj)
        want = torch.sigmoid(_B(p, nl - 1))
        for pos in (3, 4, 5):
            assert torch.allclose(h[0, pos], want, atol=1e-15)


def test_degree_8_gets_the_bias_only():
    p = NR.make_nfp_params(3, D, O, 1)
    A = 8
    atoms = np.full((1, A), 7, np.int32)
    adj = np.eye(A, dtype=np.float32)[None].copy()
    adj[0, 0, 1:] = 1; adj[0, 1:, 0] = 1                         # a star: the hub has seven neighbours and its self loop
    assert NR.deg_class(adj)[0].tolist() == [0] + [2] * 7
    _, h = NR.nfp_forward(p, atoms, adj)
    assert torch.allclose(h[0, 0], torch.sigmoid(_B(p, 0)), atol=1e-15)
    assert not torch.allclose(h[0, 1], torch.sigmoid(_B(p, 0)), atol=1e-3)


def test_padding_law():
    nl = 3
    p = NR.make_nfp_params(4, D, O, nl)
    store = synth.make_store(5, seed=3, n_lo=2, n_hi=9, n_mean=5)
    A = max(m.n for m in store)
    g0, _ = NR.nfp_forward(p, *NR.nfp_adj(store, A))
    g1, _ = NR.nfp_forward(p, *NR.nfp_adj(store, A + 4))
    per_pad = sum(torch.softmax(torch.sigmoid(_B(p, l)) @ p[f"read_out_layers/{l}/output_weight/W"].t()
                                + p[f"read_out_layers/{l}/output_weight/b"], dim=0) for l in range(nl))
    assert torch.allclose(g1 - g0, (4 * per_pad).expand_as(g0), atol=1e-12)


def test_atom_permutation_invariance():
    p = NR.make_nfp_params(5, D, O, 2)
    store = synth.make_store(3, seed=8, n_lo=4, n_hi=10, n_mean=7)
    atoms, adj = NR.nfp_adj(store)
    g, _ = NR.nfp_forward(p, atoms, adj)
    perm = np.random.RandomState(0).permutation(atoms.shape[1])
    g2, _ = NR.nfp_forward(p, atoms[:, perm], adj[:, perm][:, :, perm])
    assert torch.allclose(g, g2, atol=1e-12)


def test_asymmetric_adjacency_takes_the_class_from_the_column_sum():
    p = NR.make_nfp_params(6, D, O, 1)
    atoms = np.array([[6, 7, 8]], np.int32)
    adj = np.array([[[1, 1, 1], [0, 1, 0], [0, 0, 1]]], np.float32)      # row sums 3 1 1, column sums 1 2 2
    assert NR.deg_class(adj)[0].tolist() == [1, 2, 2]
    _, h = NR.nfp_forward(p, atoms, adj)
    E = p["embed/W"]
    want0 = torch.sigmoid((E[6] + E[7] + E[8]) @ p["layers/0/graph_linears/0/W"].t() + _B(p, 0))   # row gather, class 1
    want1 = torch.sigmoid(E[7] @ p["layers/0/graph_linears/1/W"].t() + _B(p, 0))                    # own row only, class 2
    assert torch.allclose(h[0, 0], want0, atol=1e-14) and torch.allclose(h[0, 1], want1, atol=1e-14)


def test_golden_vectors():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nfp_small.npz"))
    p = {k[2:]: T(z[k]) for k in z.files if k.startswith("p:")}
    g, h = NR.nfp_forward(p, z["atoms"], z["adj"])
    assert np.abs(g.numpy() - z["g"]).max() < 1e-12 and np.abs(h.numpy() - z["atoms_out"]).max() < 1e-12
