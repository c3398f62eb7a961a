"""CPU checks of the NFP batch side (bmp/nfp.py): the host derivation of self_w / deg_class / deg_rows against a plain
numpy computation on the dense arrays, the dense (mb, A, A) packer, the float64 PACKED formulation against the dense
restatement (values and every gradient, 1e-12), and the public symbols (module construction needs no GPU)."""
import numpy as np
import pytest
import torch

import nfp_ref as NR
from bmp import synth, packed

T = torch.from_numpy


@pytest.fixture(scope="module")
def batch():
    store = synth.make_store(40, seed=9, n_lo=2, n_hi=30, n_mean=10)
    store.append(synth.Molecule(np.array([8], np.int32), np.zeros((0, 3), np.int32)))                    # a single atom: class 1
    hub = synth.Molecule(np.full(8, 6, np.int32), np.array([[0, k, 0] for k in range(1, 8)], np.int32))  # degree 8: class 0
    store.append(hub)
    rs = np.random.RandomState(2)
    i1, i2 = np.concatenate((rs.randint(0, 40, 11), [40, 41])), np.concatenate((rs.randint(0, 40, 11), [41, 40]))
    pb = packed.pack_from_store(packed.MolStore(store), [i1, i2], device="cpu", with_dense_map=True)
    return store, i1, i2, pb


def test_host_derivation_matches_dense(batch):
    from bmp.nfp import nfp_derived
    store, i1, i2, pb = batch
    nd = nfp_derived(pb)
    N = pb.n_rows
    want_sw = np.zeros(N, np.float32); want_cls = np.zeros(N, np.int32)
    for s, idx in enumerate((i1, i2)):
        atoms, adj = NR.nfp_adj([store[k] for k in idx])
        # the same arrays from the project's dense collate: any bond type counts once, identity on the real atoms
        a4, j4 = synth.concat_mols([store[k] for k in idx])
        A = a4.shape[1]
        assert np.array_equal(a4, atoms) and np.array_equal((j4.sum(axis=1) > 0) + np.eye(A, dtype=np.float32) * (a4 != 0)[:, :, None], adj)
        dm = pb.dense_maps[s].numpy()
        real = atoms != 0
        want_sw[dm[real]] = adj[:, np.arange(adj.shape[1]), np.arange(adj.shape[1])][real]
        want_cls[dm[real]] = NR.deg_class(adj).numpy()[real]
        assert (NR.deg_class(adj).numpy()[~real] == 0).all()
    assert np.array_equal(nd["self_w"].numpy(), want_sw)
    assert np.array_equal(nd["deg_class"].numpy(), want_cls)
    assert set(np.unique(want_cls)) >= {0, 1, 2, 3, 4}
    idx, cnt = nd["deg_rows"].numpy().reshape(7, N), nd["deg_cnt"].numpy()
    for k in range(1, 8):
        rows = np.nonzero(want_cls == k)[0]
        assert cnt[k - 1] == len(rows) and np.array_equal(idx[k - 1, :len(rows)], rows)


def test_dense_packer_matches_store_packer(batch):
    from bmp.nfp import nfp_derived, pack_nfp_dense
    store, i1, i2, pb = batch
    dense = [NR.nfp_adj([store[k] for k in idx]) for idx in (i1, i2)]
    pd = pack_nfp_dense([a for a, _ in dense], [j for _, j in dense])
    for f in ("atom_id", "row_w", "csr_ptr", "csrT_ptr", "csr_val", "csrT_val", "mol_row0", "mol_nrows"):
        assert torch.equal(getattr(pd, f), getattr(pb, f)), f
    assert torch.equal(pd.csr_col >> 2, pb.csr_col >> 2) and torch.equal(pd.csrT_col >> 2, pb.csrT_col >> 2)
    a, b = nfp_derived(pd), nfp_derived(pb)
    for f in ("self_w", "deg_class", "deg_cnt"):
        assert torch.equal(a[f], b[f]), f


@pytest.mark.parametrize("d,o,nl", [(16, 8, 3)])
def test_packed_formulation_matches_dense(batch, d, o, nl):
    from bmp.nfp import nfp_derived
    store, i1, i2, pb = batch
    nd = nfp_derived(pb)
    p = {k: v.requires_grad_() for k, v in NR.make_nfp_params(7, d, o, nl).items()}
    dense = [NR.nfp_adj([store[k] for k in idx]) for idx in (i1, i2)]
    outs = [NR.nfp_forward(p, a, j) for a, j in dense]
    g_ref = torch.cat([g for g, _ in outs])
    gen = torch.Generator().manual_seed(1)
    cg = torch.randn(g_ref.shape, dtype=torch.float64, generator=gen)
    ca = [torch.randn(h.shape, dtype=torch.float64, generator=gen) for _, h in outs]
    (g_ref * cg).sum().add(sum((h * c).sum() for (_, h), c in zip(outs, ca))).backward()
    want = {k: v.grad.clone() for k, v in p.items()}
    for v in p.values():
        v.grad = None
    g, h = NR.nfp_forward_packed(p, pb, nd)
    assert (g - g_ref).abs().max() < 1e-12
    for s in (0, 1):
        assert (pb.to_dense(h, s) - outs[s][1]).abs().max() < 1e-12
    (g * cg).sum().add(sum((pb.to_dense(h, s) * ca[s]).sum() for s in (0, 1))).backward()
    for k, v in p.items():
        assert (v.grad - want[k]).abs().max() <= 1e-12 * max(1.0, want[k].abs().max().item()), k


def test_asymmetric_dense_adjacency_keeps_column_and_row_apart():
    from bmp.nfp import nfp_derived, pack_nfp_dense
    atoms = np.array([[6, 7, 8, 0]], np.int32)
    adj = np.zeros((1, 4, 4), np.float32)
    adj[0, :3, :3] = [[1, 1, 1], [0, 1, 0], [0, 0, 1]]
    pb = pack_nfp_dense([atoms], [adj])
    nd = nfp_derived(pb)
    dm = pb.dense_maps[0].numpy()[0]
    assert nd["deg_class"].numpy()[dm].tolist() == [1, 2, 2, 0] and nd["self_w"].numpy()[dm].tolist() == [1, 1, 1, 0]
    p = NR.make_nfp_params(6, 8, 4, 2)
    g_ref, h_ref = NR.nfp_forward(p, atoms, adj)
    g, h = NR.nfp_forward_packed(p, pb, nd)
    assert (g - g_ref).abs().max() < 1e-12 and (pb.to_dense(h, 0) - h_ref).abs().max() < 1e-12


def test_dense_batch_keeps_its_nfp_rows_through_replace():
    """self_w / deg_class of a dense-packed batch are fields of the batch: a dataclasses.replace that clears the derived-data
    cache (moving the batch, swapping edge values) keeps them, and nfp_derived never falls back to the store derivation."""
    import dataclasses
    from bmp.nfp import nfp_derived, pack_nfp_dense
    atoms = np.array([[6, 7, 8, 0]], np.int32)
    adj = np.zeros((1, 4, 4), np.float32)
    adj[0, :3, :3] = [[2, 1, 1], [0, 1, 0], [0, 0, 1]]
    pb = pack_nfp_dense([atoms], [adj])
    want = nfp_derived(pb)
    pb2 = dataclasses.replace(pb, _cache={})
    got = nfp_derived(pb2)
    dm = pb.dense_maps[0].numpy()[0]
    assert got["self_w"].numpy()[dm].tolist() == [2, 1, 1, 0] and got["deg_class"].numpy()[dm].tolist() == [2, 2, 2, 0]
    assert torch.equal(got["self_w"], want["self_w"]) and torch.equal(got["deg_class"], want["deg_class"])


def test_pad_like_position_with_a_column_stays_a_row():
    from bmp.nfp import nfp_derived, pack_nfp_dense
    atoms = np.array([[6, 7, 0, 0, 0]], np.int32)
    adj = np.zeros((1, 5, 5), np.float32)
    adj[0, 0, 0] = adj[0, 1, 1] = adj[0, 0, 1] = adj[0, 1, 0] = 1
    adj[0, 0, 2] = adj[0, 0, 3] = 1                                   # atom 0 points at two id-0 positions with empty rows
    pb = pack_nfp_dense([atoms], [adj])
    assert pb.mol_nrows.tolist() == [5] and pb.row_w[pb.dense_maps[0][0, 4]].item() == 1.0      # only position 4 is padding
    p = NR.make_nfp_params(6, 8, 4, 2)
    g_ref, h_ref = NR.nfp_forward(p, atoms, adj)
    g, h = NR.nfp_forward_packed(p, pb, nfp_derived(pb))
    assert (g - g_ref).abs().max() < 1e-12 and (pb.to_dense(h, 0) - h_ref).abs().max() < 1e-12


def test_public_symbols_without_a_gpu():
    from models.models import NFP, GGNN
    from bmp.relgcn import GGNNModular
    assert GGNN is GGNNModular                                       # (models/models/__init__.py of the reference exports both)
    from models.models.nfp import NFPReadout, NFPUpdate
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict, param_dict
    enc = NFP(out_dim=12, hidden_dim=24, n_layers=2)
    assert isinstance(enc.layers[0], NFPUpdate) and isinstance(enc.read_out_layers[1], NFPReadout)
    p = NR.make_nfp_params(3, 24, 12, 2)
    load_param_dict(enc, p)                                          # strict: the names are the reference's link paths
    back = param_dict(enc)
    assert set(back) == set(p) and all(torch.equal(back[k], p[k].float()) for k in p)
    assert NFP(out_dim=16).hidden_dim == 16 and not enc.plannable()
    with pytest.raises(NotImplementedError, match="nfp.py:173"):
        NFP(out_dim=8, concat_hidden=True)
    with pytest.raises(NotImplementedError):
        NFP(out_dim=8, max_degree=4)
    m = build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=2, attn="nie", encoder="nfp")
    assert isinstance(m.graph_conv, NFP) and m.attn is not None
    m = build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=2, attn=None, encoder="nfp")
    assert m.attn is None and m.mlp is not None
