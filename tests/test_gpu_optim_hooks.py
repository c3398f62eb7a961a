"""Chainer's optimizer hooks on FlatAdam's GPU path (bmp_grad_sumsq_partials + bmp_adam_step_hooked; train_binary.py:538-543):
the clip's norm against float64, the hooked update against the float64 restatement of tests/test_optim_hooks.py, the
no-hook step unchanged, a whole planned step against the dense oracle, the recorded step (GraphedTrainStep) and two ranks."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from parity_util import close                                     # noqa: E402
from test_optim_hooks import CASES, MAKE, restate_hooks, restate_steps   # noqa: E402


def dev():
    assert torch.cuda.is_available(), "GPU test selected without a GPU"
    return torch.device("cuda:0")


def _lib():
    from bmp import _lib as L
    return L


def _norm_on_device(g, gscale):
    """partials + the finalisation of bmp_adam_step_hooked (clip only, norm_out): (norm, partials)."""
    L = _lib()
    n = g.numel()
    parts = torch.full((256,), float("nan"), device=g.device)
    out = torch.zeros(1, device=g.device)
    p, m, v = (torch.zeros(n, device=g.device) for _ in range(3))
    L.check(L.lib().bmp_grad_sumsq_partials(L.ptr(parts), L.ptr(g), None, n, gscale, 0.0, 0.0, None, 1, L.stream()),
            "bmp_grad_sumsq_partials")
    L.check(L.lib().bmp_adam_step_hooked(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, gscale,
                                         1.0, 0.0, 0.0, None, 1, L.ptr(parts), L.ptr(out), L.stream()), "bmp_adam_step_hooked")
    return out, parts


@pytest.mark.parametrize("n", [1, 3, 255, 256, 4097, 52978, 322642, 5000003])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_norm_matches_fp64(n, offset, gscale):
    gen = torch.Generator().manual_seed(n)
    host = torch.randn(n + offset, generator=gen) * torch.exp(torch.randn(n + offset, generator=gen))    # spread magnitudes
    buf = host.to(dev())
    g = buf[offset:]                                               # offset 1: a view that starts mid-vector
    norm, parts = _norm_on_device(g, gscale)
    want = float(np.sqrt(np.sum((host[offset:].double().numpy() * gscale) ** 2)))
    got = float(norm.item())
    assert abs(got - want) <= 1e-6 * want, (got, want)
    P = min(256, max(1, -(-n // 2048)))
    assert torch.isfinite(parts[:P]).all() and torch.isnan(parts[P:]).all()     # P blocks, each one partial, nothing past
    norm2, parts2 = _norm_on_device(g, gscale)                     # reproducible: call to call
    assert torch.equal(norm, norm2) and torch.equal(parts[:P], parts2[:P])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                     # ... and stream to stream
        norm3, parts3 = _norm_on_device(g, gscale)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(norm, norm3) and torch.equal(parts[:P], parts3[:P])


def _flat_module():
    torch.manual_seed(7)
    return torch.nn.Sequential(torch.nn.Linear(100, 300), torch.nn.Linear(300, 17)).to(dev())      # 35417 floats


@pytest.mark.parametrize("case", sorted(CASES))
def test_hooked_adam_matches_restatement(case):
    from bmp.dp import FlatAdam
    hooks, wd, zero = CASES[case]
    hooks = [(k, 60.0 if (k == "clip" and v < 1e6) else v) for k, v in hooks]      # thresholds for this gradient (|g| ~ 90)
    opt = FlatAdam(_flat_module(), alpha=3e-3, weight_decay_rate=wd)
    n = opt.flat.numel()
    with torch.no_grad():
        opt.flat[::7] = 0.0
    for kind, val in hooks:
        opt.add_hook(MAKE[kind](val))
    p0 = opt.flat.detach().cpu().clone().numpy()
    gen = torch.Generator().manual_seed(3)
    grads = [torch.zeros(n) if zero else torch.randn(n, generator=gen) for _ in range(3)]
    for g in grads:
        opt.grad.copy_(g.to(dev()))
        opt._gscale = 0.5                                          # the 1/W that all_reduce_grads folds into the launch
        opt.step()
    p, m, v = restate_steps(p0, [0.5 * g.double().numpy() for g in grads], hooks, 3e-3, wd, fp32_args=True)
    T = torch.from_numpy
    close(opt.flat, T(p), f"hooked Adam {case}: parameters", tol=1e-6)
    close(opt.m, T(m), f"hooked Adam {case}: m", tol=1e-6, floor=1e-30)
    close(opt.v, T(v), f"hooked Adam {case}: v", tol=1e-6, floor=1e-30)


def test_no_hooks_is_the_plain_adam_launch():
    from bmp.dp import FlatAdam, GradientClipping
    L = _lib()
    opt = FlatAdam(_flat_module(), alpha=1e-2, weight_decay_rate=1e-3)
    opt.add_hook(GradientClipping(1.0))
    opt.remove_hook("GradientClipping")
    p, m, v = opt.flat.clone(), opt.m.clone(), opt.v.clone()
    gen = torch.Generator().manual_seed(4)
    for t in range(1, 4):
        g = torch.randn(opt.flat.numel(), generator=gen).to(dev())
        opt.grad.copy_(g)
        opt.step()
        a_t = 1e-2 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        L.check(L.lib().bmp_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), a_t, None, 0.9, 0.999, 1e-8, 1e-3,
                                      1.0, L.stream()), "bmp_adam_step")
    assert torch.equal(opt.flat, p) and torch.equal(opt.m, m) and torch.equal(opt.v, v)


# ---- a whole planned step against the dense float64 oracle (tests/test_gpu_planned_oracle.py) ----
OR_CFGS = {
    "c2": (dict(hidden_dim=128, out_dim=128, n_layers=4, attn="nie", head=8), {}),
    "ref_ntn": (dict(hidden_dim=32, out_dim=16, n_layers=8, weight_tying=False, attn="nie", head=8, sim_method="ntn", mlp_hidden=()),
                dict(weight_tying=False, sim_method="ntn", mlp_hidden=0)),
}


@pytest.mark.parametrize("name", sorted(OR_CFGS))
def test_hooked_step_matches_the_oracle(name):
    from bmp import packed, synth
    from bmp.dp import FlatAdam, GradientClipping, Lasso, WeightDecay
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    from oracle import ref_cpu as O
    from test_gpu_planned_oracle import _oracle_step
    kw, okw = OR_CFGS[name]
    store = synth.make_store(60, seed=23, n_lo=3, n_hi=70, n_mean=22)
    ms = packed.MolStore(store)
    rs = np.random.RandomState(8)
    B = 32
    i1, i2 = rs.randint(0, 60, B), rs.randint(0, 60, B)
    lab = rs.randint(0, 2, (B, 1)).astype(np.int32)
    a1, j1 = synth.concat_mols([store[k] for k in i1]); a2, j2 = synth.concat_mols([store[k] for k in i2])
    p = O.make_pair_params(777, encoder="ggnn", dtype=torch.float64, bias_scale=0.05, **kw)
    alpha = 1e-2
    _, _, g_o, _ = _oracle_step(p, (a1, j1, a2, j2, lab), "ggnn", kw["n_layers"], "nie", alpha, **okw)

    model = build_pair_predictor(encoder="ggnn", **kw).to(dev())
    load_param_dict(model, p)
    opt = FlatAdam(model, alpha=alpha)
    keys = [nm.replace(".", "/") for nm in opt.names]
    g_flat = torch.cat([g_o[k].reshape(-1) for k in keys]).numpy()
    p_flat = torch.cat([p[k].float().double().reshape(-1) for k in keys]).numpy()
    thr = 0.5 * float(np.sqrt(np.sum(g_flat ** 2)))                # clipping at half the measured norm: it bites
    hooks = [("clip", thr), ("decay", 5e-4), ("lasso", 1e-5)]
    opt.add_hook(GradientClipping(thr)); opt.add_hook(WeightDecay(5e-4)); opt.add_hook(Lasso(1e-5))
    p_new, _, _ = restate_steps(p_flat, [g_flat], hooks, alpha, 0.0)
    gh = restate_hooks(g_flat, p_flat, hooks)

    pb, t = packed.pack_from_store_device(packed.DeviceMolStore(ms, dev()), [i1, i2], labels=lab)
    loss = opt.functional_loss(pb, t=t)
    assert opt.plan is not None
    loss.backward()
    opt.collect_grads()
    opt.step()
    upd = opt.flat.detach().double().cpu().numpy() - p_flat
    upd_o = p_new - p_flat
    off = 0
    for pname, shp in zip(opt.names, opt.shapes):
        n = int(np.prod(shp))
        sl = slice(off, off + n)
        big = np.abs(gh[sl]) > 1e-3 * max(np.abs(gh[sl]).max(), 1e-30)      # sign(g) is ill-conditioned at g ~ 0
        if big.any():
            assert np.abs(upd[sl] - upd_o[sl])[big].max() <= 1e-3 * alpha, pname
        off += n


# ---- the recorded step (tests/test_gpu_static_batch.py) ----
ST_CFGS = {
    "c2": dict(hidden_dim=128, out_dim=128, n_layers=4, attn="nie"),
    "ref_ntn": dict(hidden_dim=32, out_dim=16, n_layers=8, attn="nie", weight_tying=False, sim_method="ntn", mlp_hidden=()),
}


@pytest.mark.parametrize("name", sorted(ST_CFGS))
def test_recorded_step_with_hooks(name):
    from bmp import packed, synth
    from bmp.dp import FlatAdam, GradientClipping, GraphedTrainStep, Lasso, WeightDecay
    from bmp.predictor import build_pair_predictor
    store = synth.make_store(120, seed=3, n_lo=3, n_hi=120, n_mean=24)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev())
    rs = np.random.RandomState(8)
    B, steps = 32, 8
    i1, i2 = rs.randint(0, 120, B * steps), rs.randint(0, 120, B * steps)
    lab = (rs.uniform(size=(B * steps, 1)) < 0.35).astype(np.int32)

    def make():
        torch.manual_seed(5)
        model = build_pair_predictor(**ST_CFGS[name]).to(dev())
        opt = FlatAdam(model, alpha=1e-3)
        hooks = dict(clip=GradientClipping(0.05), decay=WeightDecay(5e-4), lasso=Lasso(1e-5))
        for h in hooks.values():
            opt.add_hook(h)
        return opt, hooks

    oe, he = make()
    og, hg = make()
    sb = packed.StaticPairBatch(ds, B)
    stepper = GraphedTrainStep(og.module, og)
    k = [0]

    def step(tag):
        sl = slice(k[0] * B, (k[0] + 1) * B)
        k[0] += 1
        pb, t = packed.pack_from_store_device(ds, [i1[sl], i2[sl]], labels=lab[sl])
        loss = oe.functional_loss(pb, t=t); loss.backward(); oe.collect_grads(); oe.step()
        sb.load([i1[sl], i2[sl]], lab[sl])
        lg = stepper(sb)
        close(lg.detach().reshape(1), loss.detach().reshape(1), f"hooked recorded step {name} ({tag}): loss", tol=1e-4)
        close(og.flat, oe.flat, f"hooked recorded step {name} ({tag}): parameters", tol=1e-4)

    for r in range(3):
        step(f"replay {r}")
    assert len(stepper.graphs) == 1 and og.t == oe.t == 3
    ox, _ = make()                                                # a third twin keeps the old values for this step
    ox.flat.copy_(oe.flat); ox.m.copy_(oe.m); ox.v.copy_(oe.v); ox.t = oe.t
    sl = slice(3 * B, 4 * B)
    pb, t = packed.pack_from_store_device(ds, [i1[sl], i2[sl]], labels=lab[sl])
    loss = ox.functional_loss(pb, t=t); loss.backward(); ox.collect_grads(); ox.step()
    for h in (he, hg):                                            # between replays: a much tighter clip, a larger decay
        h["clip"].threshold = 1e-4
        h["decay"].rate = 1e-2
    step("threshold changed")
    assert len(stepper.graphs) == 1                               # the same recording, the new values
    stale = (ox.flat - og.flat).abs().max().item()
    assert stale > 1e-6 and stale > 10 * (og.flat - oe.flat).abs().max().item()
    for o in (oe, og):
        o.remove_hook("Lasso")
    step("Lasso removed")
    assert len(stepper.graphs) == 2                               # a new recording for the new set of hooks
    for o in (oe, og):
        o.remove_hook("WeightDecay")
        o.add_hook(Lasso(3e-5), name="l1")                        # added after recording: clip, Lasso, decay
        o.add_hook(WeightDecay(2e-3))
    step("hooks added after recording")
    assert len(stepper.graphs) == 3
    assert og.t == oe.t == 6


# ---- two ranks on the GPU path (the pattern of tests/test_gpu_dp.py) ----
def _setup():
    from bmp import packed, synth
    from bmp.predictor import build_pair_predictor
    store = synth.make_store(40, seed=6, n_lo=4, n_hi=30, n_mean=12)
    ms = packed.MolStore(store)
    rs = np.random.RandomState(1)
    i1, i2 = rs.randint(0, 40, 32), rs.randint(0, 40, 32)
    lab = (rs.uniform(size=(32, 1)) < 0.4).astype(np.int32)
    torch.manual_seed(9)
    model = build_pair_predictor(hidden_dim=64, out_dim=32, n_layers=2, attn="nie", head=4).to(dev())
    return ms, i1, i2, lab, model


def _batch(ms, i1, i2, lab, sl, pad):
    from bmp import packed
    return packed.pack_from_store(ms, [i1[sl], i2[sl]], device=dev(), pad_to=pad), torch.from_numpy(lab[sl]).to(dev())


def _hooked_opt(model):
    from bmp.dp import FlatAdam, GradientClipping, Lasso, WeightDecay
    opt = FlatAdam(model, alpha=1e-2)
    opt.add_hook(GradientClipping(1e-3))
    opt.add_hook(WeightDecay(5e-4))
    opt.add_hook(Lasso(1e-5))
    return opt


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bmp.dp import shard
        ms, i1, i2, lab, model = _setup()
        n = ms.n_atoms
        pad = [int(n[i1].max()), int(n[i2].max())]
        opt = _hooked_opt(model)
        opt.broadcast_parameters(0)
        pb, t = _batch(ms, i1, i2, lab, shard(32, rank, world), pad)
        norms = []
        for _ in range(3):
            y = opt.functional_forward(pb)
            model.loss(y, t).backward()
            opt.collect_grads()
            opt.all_reduce_grads()
            norms.append(float(opt.grad.norm()) * opt._gscale)
            opt.step()
        out[rank] = (opt.flat.detach().cpu().numpy(), norms)
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_clipping_on_the_gpu_path():
    world = 2
    port = 30700 + (os.getpid() % 2000)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    (p0, norms), (p1, _) = out[0], out[1]
    assert np.array_equal(p0, p1)                                  # ranks bit-identical after three steps
    assert min(norms) > 1e-3                                       # the clip was active on every step

    ms, i1, i2, lab, model = _setup()
    n = ms.n_atoms
    pad = [int(n[i1].max()), int(n[i2].max())]
    ref = _hooked_opt(model)
    pb, t = _batch(ms, i1, i2, lab, slice(0, 32), pad)            # one rank, the whole batch
    for _ in range(3):
        y = ref.functional_forward(pb)
        model.loss(y, t).backward()
        ref.collect_grads()
        ref.step()
    want = ref.flat.detach().cpu().numpy()
    assert np.abs(p0 - want).max() <= 1e-5 * np.abs(want).max()
