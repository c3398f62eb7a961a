"""GPU parity tests of the neural-fingerprint encoder (bmp/nfp.py, csrc/bmp_nfp.hip) against the float64 dense restatement
(tests/nfp_ref.py); max-norm 1e-4 through parity_util.close unless a test says otherwise.  Index work is bit-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nfp_ref as NR                                  # noqa: E402
from oracle import ref_cpu as O                       # noqa: E402
from bmp import synth, packed                         # noqa: E402
from test_gpu_ops import close, dev, to_dev, T        # noqa: E402


@pytest.fixture(scope="module")
def pairs():
    store = synth.make_store(40, seed=9, n_lo=2, n_hi=30, n_mean=10)
    ms = packed.MolStore(store)
    rs = np.random.RandomState(2)
    i1, i2 = rs.randint(0, 40, 13), rs.randint(0, 40, 13)
    return store, i1, i2, packed.pack_from_store(ms, [i1, i2], device="cpu", with_dense_map=True)


def _ref(p, store, i1, i2, seed=5):
    outs = [NR.nfp_forward(p, *NR.nfp_adj([store[k] for k in idx])) for idx in (i1, i2)]
    g_ref = torch.cat([g for g, _ in outs])
    gen = torch.Generator().manual_seed(seed)
    cg = torch.randn(g_ref.shape, dtype=torch.float64, generator=gen)
    ca = [torch.randn(h.shape, dtype=torch.float64, generator=gen) for _, h in outs]
    ((g_ref * cg).sum() + 0.1 * sum((h * c).sum() for (_, h), c in zip(outs, ca))).backward()
    return g_ref, [h for _, h in outs], cg, ca


def _run(enc, pb, cg, ca):
    g = enc(pb)
    atoms = enc.get_atom_array()
    d = dev()
    ((g * cg.float().to(d)).sum() + 0.1 * sum((atoms.dense(s) * ca[s].float().to(d)).sum() for s in range(len(ca)))).backward()
    return g, atoms


def test_device_derivations_equal_host(pairs):
    from bmp.nfp import nfp_derived
    store, i1, i2, pb = pairs
    h, d = nfp_derived(pb), nfp_derived(to_dev(pb))
    assert torch.equal(d["self_w"].cpu(), h["self_w"]) and torch.equal(d["deg_class"].cpu(), h["deg_class"])
    cnt = d["deg_cnt"].cpu()
    assert torch.equal(cnt, h["deg_cnt"])
    N = pb.n_rows
    di, hi = d["deg_rows"].cpu().view(7, N), h["deg_rows"].view(7, N)
    for k in range(7):
        assert torch.equal(di[k, :cnt[k]], hi[k, :cnt[k]])


def test_deg_rows_across_blocks_equal_host():
    """Three 256-row blocks and every class 0..7 (the batch above has 1.5 blocks and no row of class 1, 6 or 7): the
    offsets a block takes from the blocks in front of it, for all seven lists."""
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    from bmp.nfp import deg_rows_host
    N = 768
    cls = np.random.RandomState(11).randint(0, 8, N).astype(np.int32)
    cls[:8] = np.arange(8)
    L = _lib.lib()
    dc = torch.from_numpy(cls).to(dev())
    idx = torch.full((7 * N,), -1, dtype=torch.int32, device=dev())
    cnt = torch.empty(7, dtype=torch.int32, device=dev())
    ws = torch.empty(int(L.bmp_nfp_deg_rows_ws_ints(N)), dtype=torch.int32, device=dev())
    check(L.bmp_nfp_deg_rows(ptr(dc), N, ptr(idx), ptr(cnt), ptr(ws), stream()), "bmp_nfp_deg_rows")
    hi, hc = deg_rows_host(cls)
    assert np.array_equal(cnt.cpu().numpy(), hc) and hc.min() > 0
    assert np.array_equal(idx.cpu().numpy().reshape(7, N), hi)          # (rows past a list's count stay untouched: -1)


@pytest.mark.parametrize("hidden,out,layers", [(16, 16, 4), (24, 12, 2), (64, 32, 3), (128, 128, 4)])
def test_nfp_matches_dense_restatement(pairs, hidden, out, layers):
    from bmp.nfp import NFP
    from bmp.snapshot import load_param_dict, grad_dict
    store, i1, i2, pb = pairs
    p = {k: v.requires_grad_() for k, v in NR.make_nfp_params(3, hidden, out, layers).items()}
    g_ref, at, cg, ca = _ref(p, store, i1, i2)
    enc = NFP(out_dim=out, hidden_dim=hidden, n_layers=layers).to(dev())
    load_param_dict(enc, p)
    g, atoms = _run(enc, to_dev(pb), cg, ca)
    close(g, g_ref, "g"); close(atoms.dense(0), at[0], "atoms 1"); close(atoms.dense(1), at[1], "atoms 2")
    for name, gr in grad_dict(enc).items():
        close(gr, p[name].grad, f"grad {name}")


def test_dense_call_form_equals_packed_form(pairs):
    from bmp.nfp import NFP
    from bmp.snapshot import load_param_dict, grad_dict
    store, i1, i2, _ = pairs
    p = NR.make_nfp_params(4, 16, 8, 2)
    pb = packed.pack_from_store(packed.MolStore(store), [i1], device=dev(), with_dense_map=True)
    atoms, adj = NR.nfp_adj([store[k] for k in i1])
    res = []
    for form in ("packed", "dense"):
        enc = NFP(out_dim=8, hidden_dim=16, n_layers=2).to(dev())
        load_param_dict(enc, p)
        g = enc(pb) if form == "packed" else enc(atoms, T(adj))
        a = enc.get_atom_array().dense(0)
        (g.sum() + a.sum()).backward()
        res.append((g, a, grad_dict(enc)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


def test_asymmetric_adjacency_matches_restatement():
    from bmp.nfp import NFP
    from bmp.snapshot import load_param_dict, grad_dict
    rs = np.random.RandomState(3)
    mb, A = 4, 7
    atoms = rs.choice([6, 7, 8], size=(mb, A)).astype(np.int32); atoms[:, 5:] = 0
    adj = (rs.uniform(size=(mb, A, A)) < 0.35).astype(np.float32)
    adj[:, 5:, :] = 0; adj[:, :, 5:] = 0
    assert (adj.sum(1) != adj.sum(2)).any()
    p = {k: v.requires_grad_() for k, v in NR.make_nfp_params(8, 16, 8, 3).items()}
    g_ref, h_ref = NR.nfp_forward(p, atoms, adj)
    gen = torch.Generator().manual_seed(2)
    cg = torch.randn(g_ref.shape, dtype=torch.float64, generator=gen); ca = torch.randn(h_ref.shape, dtype=torch.float64, generator=gen)
    ((g_ref * cg).sum() + (h_ref * ca).sum()).backward()
    enc = NFP(out_dim=8, hidden_dim=16, n_layers=3).to(dev())
    load_param_dict(enc, p)
    g = enc(atoms, adj)
    a = enc.get_atom_array().dense(0)
    ((g * cg.float().to(dev())).sum() + (a * ca.float().to(dev())).sum()).backward()
    close(g, g_ref, "g"); close(a, h_ref, "atoms")
    for name, gr in grad_dict(enc).items():
        close(gr, p[name].grad, f"grad {name}")


def test_fused_and_generic_paths_agree_at_d64(pairs, monkeypatch):
    """The fused per-tile MFMA kernels (layer forward / backward, readout, listed weight gradient) against the row-wise
    kernels, forced through the modules' private switch, at d = 64 on the same batch: g, the atom states and every gradient
    at 1e-5 of the tensor's max (both f32, different summation orders).  The two runs must really take the two paths: the
    autograd functions count their forward calls per kernel form, and the results must not be bit-equal."""
    from bmp import functional as Fn
    from bmp.nfp import NFP, NFPReadout, NFPUpdate
    from bmp.snapshot import load_param_dict, grad_dict
    store, i1, i2, pb = pairs
    p = NR.make_nfp_params(5, 64, 32, 3)
    gen = torch.Generator().manual_seed(9)
    cg = torch.randn(26, 32, dtype=torch.float64, generator=gen)
    res = []
    for fused in (True, False):
        monkeypatch.setattr(NFPUpdate, "_fused", fused); monkeypatch.setattr(NFPReadout, "_fused", fused)
        before = dict(Fn.NFP_PATHS)
        enc = NFP(out_dim=32, hidden_dim=64, n_layers=3).to(dev())
        load_param_dict(enc, p)
        g = enc(to_dev(pb))
        a = enc.get_atom_array().rows
        ((g * cg.float().to(dev())).sum() + 0.1 * a.sum()).backward()
        took = {k: Fn.NFP_PATHS[k] - before[k] for k in before}
        want = {"layer_tile": 3, "readout_tile": 3, "layer_rows": 0, "readout_rows": 0} if fused else \
               {"layer_tile": 0, "readout_tile": 0, "layer_rows": 3, "readout_rows": 3}
        assert took == want, took
        res.append((g.detach(), a.detach(), grad_dict(enc)))
    close(res[0][0], res[1][0], "fused vs generic g", tol=1e-5)
    close(res[0][1], res[1][1], "fused vs generic atoms", tol=1e-5)
    for k in res[0][2]:
        close(res[0][2][k], res[1][2][k], f"fused vs generic grad {k}", tol=1e-5)
    assert not torch.equal(res[0][2]["layers/0/graph_linears/2/W"], res[1][2]["layers/0/graph_linears/2/W"])
    assert not torch.equal(res[0][1], res[1][1])


def test_smallest_readout_width_and_pad_position_with_a_column():
    """out_size 4 (the smallest width the readout accepts), and a dense adjacency in which two id-0 positions with empty rows
    are pointed at by a real atom (non-zero columns): they stay rows of their own, and everything matches the restatement."""
    from bmp.nfp import NFP, nfp_derived, pack_nfp_dense
    from bmp.snapshot import load_param_dict, grad_dict
    atoms = np.array([[6, 7, 0, 0, 0], [8, 6, 6, 0, 0]], np.int32)
    adj = np.zeros((2, 5, 5), np.float32)
    adj[0, 0, 0] = adj[0, 1, 1] = adj[0, 0, 1] = adj[0, 1, 0] = 1; adj[0, 0, 2] = adj[0, 0, 3] = 1
    adj[1, :3, :3] = 1
    pb = pack_nfp_dense([atoms], [adj])
    assert pb.mol_nrows.tolist() == [5, 4] and pb.row_w[pb.dense_maps[0][0, 4]] == 1
    p = {k: v.requires_grad_() for k, v in NR.make_nfp_params(12, 16, 4, 2).items()}
    g_ref, h_ref = NR.nfp_forward(p, atoms, adj)
    cg = torch.randn(g_ref.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))      # (g.sum() is constant in W_o)
    ((g_ref * cg).sum() + (h_ref * h_ref).sum()).backward()
    enc = NFP(out_dim=4, hidden_dim=16, n_layers=2).to(dev())
    load_param_dict(enc, p)
    g = enc(to_dev(pb))                          # (the batch's self_w / deg_class travel with it as fields)
    a = enc.get_atom_array().dense(0)
    ((g * cg.float().to(dev())).sum() + (a * a).sum()).backward()
    close(g, g_ref, "g"); close(a, h_ref, "atoms")
    for name, gr in grad_dict(enc).items():
        close(gr, p[name].grad, f"grad {name}")


def _pair_ref(p, store, i1, i2, lab, attn, A1=None, A2=None):
    enc_p = {k[len("graph_conv/"):]: v for k, v in p.items() if k.startswith("graph_conv/")}
    g1, at1 = NR.nfp_forward(enc_p, *NR.nfp_adj([store[k] for k in i1], A1))
    g2, at2 = NR.nfp_forward(enc_p, *NR.nfp_adj([store[k] for k in i2], A2))
    if attn == "nie":
        g1, g2 = O.nie_coattention(p, at1, at2, "tanh", prefix="attn/")
    y = O.mlp_forward(p, torch.cat((g1, g2), dim=-1), 2)
    return y, O.sigmoid_cross_entropy(y, T(lab))


def _pair_params(seed, hidden, out, layers, attn):
    dr = O._Draw(seed, torch.float64, 0.1)
    if attn == "nie":
        O.init_nie(dr, "attn/", hidden, out, 8)
    O.init_mlp(dr, "mlp/", 2 * out, 1, (32, 16))
    p = dict(dr.p)
    p.update(NR.make_nfp_params(seed + 1, hidden, out, layers, prefix="graph_conv/"))
    return p


@pytest.mark.parametrize("attn", ["nie", None])
def test_pair_predictor_and_three_adam_steps(pairs, attn):
    from bmp.dp import FlatAdam
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    store, i1, i2, pb = pairs
    hidden, out, layers, alpha = 16, 16, 2, 1e-2
    lab = np.random.RandomState(4).randint(0, 2, (13, 1)).astype(np.int32)
    p0 = _pair_params(21, hidden, out, layers, attn)
    names = sorted(p0)
    model = build_pair_predictor(hidden_dim=hidden, out_dim=out, n_layers=layers, attn=attn, encoder="nfp").to(dev())
    load_param_dict(model, p0)
    opt = FlatAdam(model, alpha=alpha)
    t = T(lab).to(dev())
    cur = {n: p0[n].clone() for n in names}
    state = [dict(m=torch.zeros_like(cur[n]), v=torch.zeros_like(cur[n])) for n in names]
    for step in range(1, 4):
        q = {n: cur[n].clone().requires_grad_() for n in names}
        y_o, loss_o = _pair_ref(q, store, i1, i2, lab, attn)
        # (the fine co-attention replaces the encoder's molecule vectors without reading them: the readout weights get no gradient)
        gr = torch.autograd.grad(loss_o, [q[n] for n in names], allow_unused=True)
        g_o = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, gr)}
        y = opt.functional_forward(to_dev(pb))
        loss = model.loss(y, t)
        loss.backward()
        opt.collect_grads()
        if step == 1:
            close(y, y_o, "logits"); close(loss, loss_o, "loss")
            off = 0
            for name, shp in zip(opt.names, opt.shapes):
                n = int(np.prod(shp))
                close(opt.grad[off:off + n].view(shp), g_o[name.replace(".", "/")], f"grad {name}")
                off += n
        opt.step()
        O.chainer_adam_step([cur[n] for n in names], [g_o[n] for n in names], state, step, alpha=alpha)
    off = 0
    for name, shp in zip(opt.names, opt.shapes):
        n = int(np.prod(shp))
        close(opt.flat[off:off + n].view(shp), cur[name.replace(".", "/")], f"param after 3 steps {name}")
        off += n


def test_full_size_batch_d128():
    """1024 pairs of the DDI-shaped synthetic store, d = 128, NFP + MLP: the labels of all but a handful of pairs are -1, so
    the loss and every gradient equal the restatement's on those pairs padded to the batch's A1 / A2.  The handful holds the
    largest and the smallest molecule, a single-atom molecule (class 1) and a hub atom of degree 8 (class 0) appended to the
    store, and between them every degree class of the batch.  Two runs give bit-identical gradients."""
    from bmp.nfp import nfp_derived
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict, grad_dict
    B, hidden, out, layers = 1024, 128, 128, 4
    store = synth.make_store(544, seed=2018)
    store.append(synth.Molecule(np.array([8], np.int32), np.zeros((0, 3), np.int32)))
    store.append(synth.Molecule(np.full(8, 6, np.int32), np.array([[0, k, 0] for k in range(1, 8)], np.int32)))
    i1, i2, _ = synth.make_pairs(544, seed=777, limit=B)
    i1, i2 = i1.copy(), i2.copy()
    i1[5], i2[5], i1[6], i2[6] = 544, 545, 545, 544
    n = np.array([m.n for m in store])
    pick = sorted({5, 6, int(np.argmax(n[i1])), int(np.argmax(n[i2])), int(np.argmin(n[i1][7:]) + 7), 100, 500, 900})
    lab = np.full((B, 1), -1, np.int32)
    lab[pick, 0] = np.random.RandomState(1).randint(0, 2, len(pick))
    ms = packed.MolStore(store)
    pb = packed.pack_from_store(ms, [i1, i2], device=dev(), with_dense_map=True)
    nd_dev = nfp_derived(pb)
    nd_host = nfp_derived(packed.pack_from_store(ms, [i1, i2], device="cpu"))
    assert torch.equal(nd_dev["self_w"].cpu(), nd_host["self_w"]) and torch.equal(nd_dev["deg_class"].cpu(), nd_host["deg_class"])
    cnt = nd_dev["deg_cnt"].cpu()
    assert torch.equal(cnt, nd_host["deg_cnt"])
    for k in range(7):                           # 58 k rows: the block-rank carry of the row lists over 228 blocks
        assert torch.equal(nd_dev["deg_rows"].cpu().view(7, -1)[k, :cnt[k]], nd_host["deg_rows"].view(7, -1)[k, :cnt[k]])
    cls = nd_dev["deg_class"].cpu().numpy()
    rows = torch.cat([pb.dense_maps[s][pick].reshape(-1) for s in (0, 1)]).cpu().numpy()
    assert set(np.unique(cls[rows])) == set(np.unique(cls)), "the chosen pairs must hold every degree class of the batch"
    assert {0, 1} <= set(np.unique(cls[rows]))
    p = _pair_params(31, hidden, out, layers, None)
    q = {k: v.clone().requires_grad_() for k, v in p.items()}
    A1, A2 = int(n[i1].max()), int(n[i2].max())
    y_o, loss_o = _pair_ref(q, store, i1[pick], i2[pick], lab[pick], None, A1, A2)
    loss_o.backward()
    t = T(lab).to(dev())
    runs = []
    for _ in range(2):
        model = build_pair_predictor(hidden_dim=hidden, out_dim=out, n_layers=layers, attn=None, encoder="nfp").to(dev())
        load_param_dict(model, p)
        y = model(pb)
        loss = model.loss(y, t)
        loss.backward()
        runs.append((y.detach(), loss.detach(), grad_dict(model)))
    y, loss, gd = runs[0]
    close(y[pick], y_o, "logits of the chosen pairs"); close(loss, loss_o, "loss")
    for name, gr in gd.items():
        close(gr, q[name].grad, f"grad {name}")
        assert torch.equal(gr, runs[1][2][name]), f"{name}: not bit-identical run to run"
