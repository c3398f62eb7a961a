"""GPU parity tests of the GGNN layer aggregators (layer_aggregator = 'concat' / 'max-pool' / 'attn').

Reference values: the float64 restatement tests/agg_ref.py (its own CPU checks: tests/test_agg_ref.py) and the committed
fixtures tests/golden/ggnn_agg_*.npz.  Tolerance: the project's 1e-4 of the tensor's max-abs; the achieved error of every
comparison is logged (parity_util)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import agg_ref as AR                              # noqa: E402
from oracle import ref_cpu as O                   # noqa: E402
from bmp import packed, synth                     # noqa: E402
from test_gpu_ops import close, dev               # noqa: E402

T_ = torch.from_numpy
MODES = {"max-pool": 0, "attn": 1}


# ----------------------------------------------------------------------------------------------- the operator alone
def _operator_case(mode, T, d, n_rows, seed):
    g = torch.Generator().manual_seed(seed)
    hs = [torch.randn(n_rows, d, generator=g) * 0.7 for _ in range(T)]
    W = torch.randn(T, T, generator=g) / np.sqrt(T)
    b = 0.3 * torch.randn(T, generator=g)
    c = torch.randn(n_rows, d, generator=g)
    return hs, W, b, c


def _operator_gpu(Fn, mode, hs, W, b, c):
    hd = [h.to(dev()).requires_grad_() for h in hs]
    Wd = W.to(dev()).requires_grad_() if mode == "attn" else None
    bd = b.to(dev()).requires_grad_() if mode == "attn" else None
    y = Fn.LayerAggFn.apply(MODES[mode], Wd, bd, *hd)
    (y * c.to(dev())).sum().backward()
    return y, hd, Wd, bd


@pytest.mark.parametrize("n_rows", [128, 300 * 128])
@pytest.mark.parametrize("d", [16, 32, 128])
@pytest.mark.parametrize("T", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", ["max-pool", "attn"])
def test_operator_against_the_restatement(mode, T, d, n_rows):
    from bmp import functional as Fn
    hs, W, b, c = _operator_case(mode, T, d, n_rows, seed=1000 * T + d)
    hr = [h.double().requires_grad_() for h in hs]
    Wr, br = W.double().requires_grad_(), b.double().requires_grad_()
    yr = AR.layer_aggregate(hr, mode, Wr, br) if mode == "attn" else AR.layer_aggregate(hr, mode)
    (yr * c.double()).sum().backward()
    tag = f"{mode} T={T} d={d} rows={n_rows}"
    y, hd, Wd, bd = _operator_gpu(Fn, mode, hs, W, b, c)
    close(y, yr, f"agg y ({tag})")
    for t in range(T):
        close(hd[t].grad, hr[t].grad, f"agg dh[{t}] ({tag})")
    if mode == "attn":
        close(Wd.grad, Wr.grad, f"agg dW ({tag})")
        close(bd.grad, br.grad, f"agg db ({tag})")
        _, _, W2, b2 = _operator_gpu(Fn, mode, hs, W, b, c)                 # a second run adds the same numbers in the same order
        assert torch.equal(W2.grad, Wd.grad) and torch.equal(b2.grad, bd.grad), f"dW / db differ between two runs ({tag})"


def test_operator_kept_softmax_gives_the_recomputed_gradients():
    """The two forms of the attn backward -- p recomputed from the step tensors (what the library's callers use) and p read
    back from the forward's aux planes -- through the C ABI directly."""
    from bmp import functional as Fn, _lib
    from bmp._lib import check, ptr, stream
    L = _lib.lib()
    T, d, N = 4, 32, 1024
    hs, W, b, c = _operator_case("attn", T, d, N, seed=9)
    hd, Wd, bd, dy = [h.to(dev()) for h in hs], W.to(dev()), b.to(dev()), c.to(dev())
    y0, y1 = torch.empty(N, d, device=dev()), torch.empty(N, d, device=dev())
    aux = torch.empty(T, N, d, device=dev())
    check(L.bmp_layer_agg_fwd(Fn._ptr_array(hd), T, N, d, 1, ptr(Wd), ptr(bd), ptr(y0), None, stream()), "fwd")
    check(L.bmp_layer_agg_fwd(Fn._ptr_array(hd), T, N, d, 1, ptr(Wd), ptr(bd), ptr(y1), ptr(aux), stream()), "fwd kept")
    assert torch.equal(y0, y1)
    close(aux.sum(dim=0), torch.ones(N, d), "kept softmax sums to one")
    nws = L.bmp_layer_agg_ws_floats(N, d, T)
    outs = []
    for a in (None, aux):
        dh = [torch.empty(N, d, device=dev()) for _ in range(T)]
        dW, db, ws = torch.empty(T, T, device=dev()), torch.empty(T, device=dev()), torch.empty(nws, device=dev())
        check(L.bmp_layer_agg_bwd(ptr(dy), Fn._ptr_array(hd), T, N, d, 1, ptr(Wd), ptr(bd), ptr(a), Fn._ptr_array(dh), ptr(dW),
                                  ptr(db), 0, ptr(ws), nws, stream()), "bwd")
        outs.append((dh, dW, db))
    for t in range(T):
        close(outs[1][0][t], outs[0][0][t], f"kept-p dh[{t}]", tol=1e-5)
    close(outs[1][1], outs[0][1], "kept-p dW", tol=1e-5)
    close(outs[1][2], outs[0][2], "kept-p db", tol=1e-5)


def test_operator_refuses_more_than_eight_tensors_and_odd_widths():
    from bmp import functional as Fn
    with pytest.raises(ValueError):
        Fn.LayerAggFn.apply(0, None, None, *[torch.zeros(128, 16, device=dev()) for _ in range(9)])
    with pytest.raises(ValueError):
        Fn.LayerAggFn.apply(0, None, None, *[torch.zeros(128, 18, device=dev()) for _ in range(2)])
    with pytest.raises(ValueError):
        Fn.LayerAggFn.apply(1, torch.zeros(3, 3, device=dev()), None, *[torch.zeros(128, 16, device=dev()) for _ in range(2)])


# ----------------------------------------------------------------------------------------------- encoder against the fixtures
FIX = {"concat": "ggnn_agg_concat.npz", "max-pool": "ggnn_agg_max.npz", "attn": "ggnn_agg_attn.npz"}


def _fixture_model(z, tag, agg, T, tied):
    from bmp.ggnn import GGNN
    from bmp.snapshot import load_param_dict
    pre = f"{tag}:p:"
    p = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    enc = GGNN(out_dim=8, hidden_dim=16, n_layers=T, n_atom_types=p["embed/W"].shape[0], layer_aggregator=agg,
               weight_tying=tied).to(dev())
    load_param_dict(enc, p)
    return enc


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("T", [3, 4])
@pytest.mark.parametrize("agg", ["concat", "max-pool", "attn"])
def test_encoder_against_the_fixture(agg, T, tied, golden_dir):
    from bmp.snapshot import grad_dict
    tag = f"c{T}{'t' if tied else 'u'}"
    with np.load(os.path.join(golden_dir, FIX[agg])) as z:
        enc = _fixture_model(z, tag, agg, T, tied)
        atoms, adj, g_ref, gw = z["atoms"], z["adj"], T_(z[f"{tag}:g"]), T_(z[f"{tag}:gw"])
        d_ref = {k[len(f"{tag}:d:"):]: T_(z[k]) for k in z.files if k.startswith(f"{tag}:d:")}
        dh0_ref = T_(z[f"{tag}:dh0"])
    assert not enc._plan_fused()                                            # d = 16: the unfused operators
    gwd = gw.float().to(dev())
    for form in ("dense", "packed"):
        enc.zero_grad()
        g = enc(atoms, adj) if form == "dense" else enc(packed.pack_from_dense([atoms], [adj], device=dev()))
        (g * gwd).sum().backward()
        close(g, g_ref, f"fixture {agg} {tag} g ({form})")
        for name, gr in grad_dict(enc).items():                             # every parameter, the embedding among them
            close(gr, d_ref[name], f"fixture {agg} {tag} grad {name} ({form})")
        with pytest.raises(RuntimeError, match="layer_aggregator"):
            enc.get_atom_array()
    # float features skip the embedding (models/ggnn.py:604-605): the gradient with respect to h0 as an input
    h0 = enc.embed.W.detach()[T_(atoms).long().to(dev())].clone().requires_grad_()
    g = enc(h0, adj)
    (g * gwd).sum().backward()
    close(g, g_ref, f"fixture {agg} {tag} g (float features)")
    close(h0.grad, dh0_ref, f"fixture {agg} {tag} dh0")


# ----------------------------------------------------------------------------------------------- encoder at the fused widths
def _synthetic(n_mols, seed, n_hi=40):
    store = synth.make_store(n_mols, seed=seed, n_lo=2, n_hi=n_hi, n_mean=12)
    return store, synth.concat_mols(store)


def _ref_grads(p, a, j, T, agg, tied, wv, masks=None):
    p = {k: v.clone().requires_grad_() for k, v in p.items()}
    g, _ = AR.ggnn_agg_forward(p, T_(a), T_(j).double(), T, agg, weight_tying=tied, dropout_masks=masks)
    grads = torch.autograd.grad((g * wv).sum(), list(p.values()))
    return g.detach(), dict(zip(p, grads))


@pytest.mark.parametrize("d,T,tied", [(32, 8, False), (64, 4, True), (128, 4, True), (48, 3, False)])
@pytest.mark.parametrize("agg", ["concat", "max-pool", "attn"])
def test_encoder_against_a_fresh_restatement_run(agg, d, T, tied):
    """Fused step kernels (d = 32, 64, 128) and the unfused operators (d = 48); the dense call form and the PackedMolBatch
    form; eval-mode dropout is the identity."""
    from bmp import functional as Fn
    from bmp.ggnn import GGNN
    from bmp.snapshot import grad_dict, load_param_dict
    store, (a, j) = _synthetic(12, seed=31 + d)
    out = 16
    p = AR.make_agg_params(5 + d, d, out, T, agg, weight_tying=tied, bias_scale=0.05)
    p = {k: v.float().double() for k, v in p.items()}
    wv = T_(np.random.RandomState(d).normal(size=(a.shape[0], out)))
    g_ref, d_ref = _ref_grads(p, a, j, T, agg, tied, wv)
    enc = GGNN(out_dim=out, hidden_dim=d, n_layers=T, layer_aggregator=agg, weight_tying=tied, dropout_rate=0.3).to(dev())
    load_param_dict(enc, p)
    enc.eval()                                                              # chainer's train=False: dropout is the identity
    assert enc._plan_fused() == (d in (32, 64, 128)) and Fn.step_supported(d) == (d in (32, 64, 128))
    ms = packed.MolStore(store)
    for form in ("dense", "packed"):
        enc.zero_grad()
        g = enc(a, j) if form == "dense" else enc(packed.pack_from_store(ms, [np.arange(len(store))], device=dev()))
        (g * wv.float().to(dev())).sum().backward()
        close(g, g_ref, f"encoder {agg} d={d} T={T} g ({form})")
        for name, gr in grad_dict(enc).items():
            close(gr, d_ref[name], f"encoder {agg} d={d} T={T} grad {name} ({form})")


@pytest.mark.parametrize("agg", ["concat", "max-pool", "attn"])
def test_encoder_with_injected_training_masks(agg):
    """F.dropout on every step output (models/ggnn.py:626-627): the aggregator sees the DROPPED outputs."""
    from bmp.ggnn import GGNN
    from bmp.snapshot import grad_dict, load_param_dict
    d, T, out, p_drop = 32, 3, 16, 0.25
    store, (a, j) = _synthetic(10, seed=21, n_hi=24)
    p = AR.make_agg_params(77, d, out, T, agg, bias_scale=0.05)
    p = {k: v.float().double() for k, v in p.items()}
    pb = packed.pack_from_dense([a], [j], device=dev())
    rs = np.random.RandomState(3)
    masks_rows = [T_((rs.uniform(size=(pb.n_rows, d)) >= p_drop).astype(np.float64) / (1.0 - p_drop)) for _ in range(T)]
    dm = pb.dense_maps[0].cpu()
    wv = T_(rs.normal(size=(a.shape[0], out)))
    g_ref, d_ref = _ref_grads(p, a, j, T, agg, True, wv, masks=[mk[dm] for mk in masks_rows])
    enc = GGNN(out_dim=out, hidden_dim=d, n_layers=T, layer_aggregator=agg, dropout_rate=p_drop).to(dev())
    load_param_dict(enc, p)
    enc.train()
    enc._dropout_masks = [mk.float().to(dev()) for mk in masks_rows]
    g = enc(pb)
    (g * wv.float().to(dev())).sum().backward()
    # (max-pool: a dropped value is exactly 0 in both runs and the kept ones are scaled alike, so the routing agrees)
    close(g, g_ref, f"dropout {agg} g")
    for name, gr in grad_dict(enc).items():
        close(gr, d_ref[name], f"dropout {agg} grad {name}")


def test_oversized_molecule_takes_the_row_wise_operators():
    """A molecule taller than a tile (the reference sets no size limit): the unfused operators, then the same aggregator."""
    from bmp.ggnn import GGNN
    from bmp.snapshot import grad_dict, load_param_dict
    d, T, out = 32, 3, 16
    rs = np.random.RandomState(4)
    n = 150
    big = synth.Molecule(rs.choice([6, 7, 8], size=n).astype(np.int32),
                         np.stack([np.arange(n - 1), np.arange(1, n), rs.randint(0, 4, n - 1)], axis=1).astype(np.int32))
    store = synth.make_store(4, seed=2, n_lo=3, n_hi=20, n_mean=8) + [big]
    a, j = synth.concat_mols(store)
    p = {k: v.float().double() for k, v in AR.make_agg_params(8, d, out, T, "attn", bias_scale=0.05).items()}
    wv = T_(rs.normal(size=(len(store), out)))
    g_ref, d_ref = _ref_grads(p, a, j, T, "attn", True, wv)
    enc = GGNN(out_dim=out, hidden_dim=d, n_layers=T, layer_aggregator="attn").to(dev())
    load_param_dict(enc, p)
    pb = packed.pack_from_store(packed.MolStore(store), [np.arange(len(store))], device=dev())
    assert pb.oversized
    g = enc(pb)
    (g * wv.float().to(dev())).sum().backward()
    close(g, g_ref, "oversized attn g")
    for name, gr in grad_dict(enc).items():
        close(gr, d_ref[name], f"oversized attn grad {name}")


# ----------------------------------------------------------------------------------------------- planned path
def _pair_world(n_store, B, seed, n_hi=44):
    store = synth.make_store(n_store, seed=seed, n_lo=2, n_hi=n_hi, n_mean=16)
    rs = np.random.RandomState(seed + 1)
    i1, i2 = rs.randint(0, n_store, B), rs.randint(0, n_store, B)
    lab = rs.randint(0, 2, (B, 1)).astype(np.int32)
    return store, i1, i2, lab


def _pair_model(agg, d, out, T, tied, sim_method, mlp_hidden, p=None):
    from bmp.ggnn import GGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.snapshot import load_param_dict
    enc = GGNN(out_dim=out, hidden_dim=d, n_layers=T, layer_aggregator=agg, weight_tying=tied)
    model = GraphConvPredictorForPair(enc, None, build_link_predictor(sim_method, out, 1, mlp_hidden)).to(dev())
    if p is not None:
        load_param_dict(model, p)
    return model


def _pair_ref(p, store, i1, i2, lab, T, agg, tied, sim_method, n_hidden):
    a1, j1 = synth.concat_mols([store[k] for k in i1]); a2, j2 = synth.concat_mols([store[k] for k in i2])
    q = {k: v.clone().requires_grad_() for k, v in p.items()}
    y = AR.pair_agg_forward(q, T_(a1), T_(j1).double(), T_(a2), T_(j2).double(), T, agg, tied, sim_method, n_hidden)
    loss = O.sigmoid_cross_entropy(y, T_(lab))
    names = sorted(q)
    grads = torch.autograd.grad(loss, [q[n] for n in names])
    return y.detach(), loss.detach(), dict(zip(names, grads))


def _flat_grads(opt):
    out, off = {}, 0
    for name, shp in zip(opt.names, opt.shapes):
        n = int(np.prod(shp))
        out[name.replace(".", "/")] = opt.grad[off:off + n].view(shp)
        off += n
    return out


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("agg", ["max-pool", "attn"])
def test_planned_equals_eager_and_tracks_adam(agg, d):
    """Under a FlatAdam plan (prepared weights, agg.dW / agg.db in the plan's buffers) the loss and the gradients are the
    autograd path's, and three Adam steps follow the restatement with oracle.ref_cpu.chainer_adam_step."""
    from bmp.dp import FlatAdam
    T, out, alpha = 4, 16, 1e-2
    store, i1, i2, lab = _pair_world(30, 12, seed=5)
    p = AR.make_agg_pair_params(11, d, out, T, agg, weight_tying=False)
    p = {k: v.float().double() for k, v in p.items()}
    model = _pair_model(agg, d, out, T, False, "mlp", (32, 16), p)
    pb = packed.pack_from_store(packed.MolStore(store), [i1, i2], device=dev())
    t = T_(lab).to(dev())
    # eager autograd path
    model.zero_grad()
    loss_e = model.loss(model(pb), t)
    loss_e.backward()
    from bmp.snapshot import grad_dict
    g_e = {k: v.clone() for k, v in grad_dict(model).items()}
    # planned path
    opt = FlatAdam(model, alpha=alpha)
    names = sorted(p)
    state = [dict(m=torch.zeros_like(p[n]), v=torch.zeros_like(p[n])) for n in names]
    bigs = {}
    for step in range(1, 4):
        loss = opt.functional_loss(pb, t=t)
        assert opt.plan is not None and "graph_conv." in opt.plan.P
        assert ("agg.W" in opt.plan.P["graph_conv."]) == (agg == "attn")
        loss.backward()
        opt.collect_grads()
        y_o, loss_o, g_o = _pair_ref(p, store, i1, i2, lab, T, agg, False, "mlp", 2)
        close(loss, loss_o, f"planned {agg} d={d} step {step}: loss")
        fg = _flat_grads(opt)
        for n in names:
            close(fg[n], g_o[n], f"planned {agg} d={d} step {step}: grad {n}")
            if step == 1:
                close(fg[n], g_e[n], f"planned against eager {agg} d={d}: grad {n}", tol=1e-5)
        if step == 1:
            close(loss, loss_e, f"planned against eager {agg} d={d}: loss", tol=1e-5)
        opt.step()
        before = {n: p[n].clone() for n in names}
        O.chainer_adam_step([p[n] for n in names], [g_o[n] for n in names], state, step, alpha=alpha)
        now = dict(zip([n.replace(".", "/") for n in opt.names], [None] * len(opt.names)))
        off = 0
        for name, shp in zip(opt.names, opt.shapes):
            n = int(np.prod(shp))
            now[name.replace(".", "/")] = opt.flat[off:off + n].view(shp).double().cpu()
            off += n
        for n in names:
            # The update alpha_t m / (sqrt(v) + eps) is at most ~ alpha in size and depends on the gradients of the steps so
            # far through m and sqrt(v).  Where every one of them is at least a tenth of its tensor's largest entry, the 1e-4
            # (of that largest entry) the gradients may differ by is 1e-3 of the element, which moves m and sqrt(v) by 1e-3
            # each: 2e-3 * alpha on the update.  Elsewhere the update turns on the sign of a gradient near zero.
            big = g_o[n].abs() > 1e-1 * g_o[n].abs().max().clamp(min=1e-30)
            bigs[n] = big if n not in bigs else (bigs[n] & big)
            if bigs[n].any():
                err = ((now[n] - before[n].float().double()) - (p[n] - before[n]))[bigs[n]].abs().max().item()
                print(f"[adam] step {step} {n}: update differs by {err:.3e} (bound {2e-3 * alpha:.1e})")
                assert err <= 2e-3 * alpha, f"Adam step {step} {n}: update differs by {err:.2e}"
        # the restatement goes on from the GPU's float32 parameters, so that the steps do not drift apart
        p = {n: now[n].clone() for n in names}


def test_planned_encoder_layout_equals_packed_batch():
    """encode_rows / readout_rows: the encoder runs on the encoder layout (every distinct molecule once), the aggregator
    there, the readout on the per-instance rows."""
    from bmp import enclayout
    from bmp.dp import FlatAdam
    store, i1, i2, lab = _pair_world(40, 32, seed=9)
    model = _pair_model("attn", 32, 16, 8, False, "hole", ())
    opt = FlatAdam(model, alpha=1e-3)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev())
    pb, t = packed.pack_from_store_device(ds, [i1, i2], labels=lab)
    loss = opt.functional_loss(pb, t=t); loss.backward(); opt.collect_grads()
    l_ref, g_ref = loss.detach().clone(), opt.grad.clone()
    eb, te = enclayout.encode_from_store_device(ds, [i1, i2], labels=lab)
    loss = opt.functional_loss(eb, t=te); loss.backward(); opt.collect_grads()
    close(loss.reshape(1), l_ref.reshape(1), "encoder layout attn: loss", tol=1e-5)
    close(opt.grad, g_ref, "encoder layout attn: flat gradient", tol=1e-5)


# ----------------------------------------------------------------------------------------------- recorded step
@pytest.mark.parametrize("sim_method", ["mlp", "hole"])
def test_recorded_step_replays_equal_launch_by_launch_steps(sim_method):
    """The model of the reference's recorded run (RECORD.txt:130: --layer-aggregator=attn --weight-tying=False
    --fp-hidden-dim=32 --conv-layers=8) as ONE HIP graph on the fixed-shape batch, replayed on different batches."""
    from bmp.dp import FlatAdam, GraphedTrainStep
    store = synth.make_store(80, seed=3, n_lo=3, n_hi=100, n_mean=24)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev())
    rs = np.random.RandomState(8)
    B, steps = 32, 6
    i1, i2 = rs.randint(0, 80, B * steps), rs.randint(0, 80, B * steps)
    lab = (rs.uniform(size=(B * steps, 1)) < 0.35).astype(np.int32)
    hidden = (32, 16) if sim_method == "mlp" else ()
    eager = _pair_model("attn", 32, 16, 8, False, sim_method, hidden)
    graphed = _pair_model("attn", 32, 16, 8, False, sim_method, hidden)
    graphed.load_state_dict(eager.state_dict())
    oe, og = FlatAdam(eager, alpha=1e-3), FlatAdam(graphed, alpha=1e-3)
    assert torch.equal(oe.flat, og.flat)
    sb = packed.StaticPairBatch(ds, B)
    stepper = GraphedTrainStep(graphed, og)
    le, lg = [], []
    for k in range(steps):
        sl = slice(k * B, (k + 1) * B)
        pb, t = packed.pack_from_store_device(ds, [i1[sl], i2[sl]], labels=lab[sl])
        loss = oe.functional_loss(pb, t=t); loss.backward(); oe.collect_grads(); oe.step()
        le.append(float(loss.detach()))
        sb.load([i1[sl], i2[sl]], lab[sl])
        lg.append(float(stepper(sb).detach()))
    assert len(stepper.graphs) == 1 and og.t == oe.t == steps
    assert "agg.W" in og.plan.P["graph_conv."]
    close(torch.tensor(lg), torch.tensor(le), f"recorded attn step ({sim_method}): losses of {steps} steps")
    close(og.flat, oe.flat, f"recorded attn step ({sim_method}): parameters after {steps} steps")
    assert not np.allclose(le[0], le[-1])


# ----------------------------------------------------------------------------------------------- full size
def _full_size(agg):
    from bmp.dp import FlatAdam
    d, T, out, B = 128, 4, 128, 1024
    store = synth.make_store(544, seed=2018)
    i1, i2, lab = synth.make_pairs(544, seed=777, limit=B)
    lab = lab.reshape(B, 1).astype(np.int32)
    p = AR.make_agg_pair_params(777, d, out, T, agg, weight_tying=True)
    p = {k: v.float().double() for k, v in p.items()}
    model = _pair_model(agg, d, out, T, True, "mlp", (32, 16), p)
    opt = FlatAdam(model, alpha=1e-3)
    pb, t = packed.pack_from_store_device(packed.DeviceMolStore(packed.MolStore(store), dev()), [i1, i2], labels=lab)
    loss = opt.functional_loss(pb, t=t)
    loss.backward()
    opt.collect_grads()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    y_o, loss_o, g_o = _pair_ref(p, store, i1, i2, lab, T, agg, True, "mlp", 2)
    return model, opt, loss, y_o, loss_o, g_o


def test_full_size_attn():
    """One 1024-pair batch of the DDI-shaped store, d = 128, T = 4, 'attn', planned path: logits, loss and every parameter
    gradient against the restatement."""
    model, opt, loss, y_o, loss_o, g_o = _full_size("attn")
    close(model.y, y_o, "full size attn: logits")
    close(loss, loss_o, "full size attn: loss")
    for n, g in _flat_grads(opt).items():
        close(g, g_o[n], f"full size attn: grad {n}")


def test_full_size_max_pool():
    """The same batch with 'max-pool': the forward and the PARAMETER gradients only.  Among the millions of elements of
    this batch some have their two largest step values closer than float32 resolves, and the float32 run may hand such an
    element's gradient to the other step than the float64 run does; each is one element's contribution to a sum over all
    rows, far below the tolerance, which stays the project's 1e-4 -- but a per-element comparison of the row gradients
    would not be a statement about the kernel."""
    model, opt, loss, y_o, loss_o, g_o = _full_size("max-pool")
    close(model.y, y_o, "full size max-pool: logits")
    close(loss, loss_o, "full size max-pool: loss")
    for n, g in _flat_grads(opt).items():
        close(g, g_o[n], f"full size max-pool: grad {n}")
