"""Chainer's optimizer hooks on FlatAdam's CPU path (train_binary.py:538-543: GradientClipping(max_norm), WeightDecay(l2_rate),
Lasso(l1_rate), added in that order) against a float64 restatement of Chainer's semantics, which is not installable here:

* hooks run before the update rule, in the order they were added, each on the gradient the earlier hooks left;
* GradientClipping(threshold): g *= min(1, threshold / sqrt(sum g^2)), a zero norm gives 1;
* WeightDecay(rate): g += rate * p;  Lasso(rate): g += rate * sign(p), sign(0) = 0  (p before the update);
* then chainer.optimizers.Adam (oracle.ref_cpu.chainer_adam_step), its own weight_decay_rate included.

Also: registration (one hook per kind, remove_hook) and two gloo ranks with clipping against one rank on the whole batch."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from bmp.dp import FlatAdam, GradientClipping, Lasso, WeightDecay, shard
from bmp.mlp import MLP
from bmp.predictor import sigmoid_cross_entropy

MAKE = {"clip": GradientClipping, "decay": WeightDecay, "lasso": Lasso}


def restate_hooks(g, p, hooks):
    """float64 numpy: the gradient after the hooks [(kind, threshold or rate), ...] in their order."""
    g = np.asarray(g, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    for kind, val in hooks:
        if kind == "clip":
            norm = np.sqrt(np.sum(g * g))
            g = g * (min(1.0, val / norm) if norm > 0 else 1.0)
        elif kind == "decay":
            g = g + val * p
        else:
            g = g + val * np.sign(p)
    return g


def restate_steps(p0, grads, hooks, alpha, wd, t0=0, fp32_args=False):
    """float64 restatement of len(grads) hooked Adam steps from p0 with zero moments: (p, m, v).  ``fp32_args``: beta1,
    beta2, eps and weight_decay_rate as the kernels receive them (rounded to fp32; 1 - fl32(0.999) differs from 0.001 by
    5e-5 relative), and alpha_t as the host computes it, from the unrounded betas."""
    from oracle.ref_cpu import chainer_adam_step
    b1, b2, eps = 0.9, 0.999, 1e-8
    r = (lambda x: float(np.float32(x))) if fp32_args else (lambda x: x)
    p = torch.from_numpy(np.asarray(p0, dtype=np.float64).copy())
    st = dict(m=torch.zeros_like(p), v=torch.zeros_like(p))
    for k, g in enumerate(grads):
        t = t0 + k + 1
        a_t = alpha * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        al = a_t * (1.0 - r(b1) ** t) / np.sqrt(1.0 - r(b2) ** t)           # chainer_adam_step's alpha_t is then a_t
        gh = torch.from_numpy(restate_hooks(g, p.numpy(), hooks))
        chainer_adam_step([p], [gh], [st], t, alpha=al, beta1=r(b1), beta2=r(b2), eps=r(eps), weight_decay_rate=r(wd))
    return p.numpy(), st["m"].numpy(), st["v"].numpy()


def _model():
    torch.manual_seed(5)
    return MLP(1, (8, 4), in_dim=16)


def _grads(n, steps=3, zero=False):
    g = torch.Generator().manual_seed(1)
    return [torch.zeros(n) if zero else torch.randn(n, generator=g) for _ in range(steps)]


CASES = {
    "clip": ([("clip", 0.5 * np.sqrt(177.0))], 0.0, False),           # bites: |g| ~ sqrt(n) = sqrt(177)
    "decay": ([("decay", 5e-2)], 0.0, False),
    "lasso": ([("lasso", 2e-2)], 0.0, False),
    "reference_order": ([("clip", 6.0), ("decay", 5e-2), ("lasso", 2e-2)], 1e-3, False),
    "decay_before_clip": ([("decay", 5e-1), ("clip", 6.0)], 0.0, False),
    "clip_inactive": ([("clip", 1e6), ("lasso", 2e-2)], 0.0, False),
    "zero_gradient": ([("clip", 1.0), ("decay", 5e-2), ("lasso", 2e-2)], 0.0, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_cpu_hooks_match_chainer_restatement(case):
    hooks, wd, zero = CASES[case]
    model = _model()
    opt = FlatAdam(model, alpha=3e-3, weight_decay_rate=wd)
    n = opt.flat.numel()
    assert n == 177
    with torch.no_grad():
        opt.flat[::7] = 0.0                                  # sign(0) = 0 for Lasso
    for kind, val in hooks:
        opt.add_hook(MAKE[kind](val))
    p0 = opt.flat.detach().clone().numpy()
    grads = _grads(n, zero=zero)
    for g in grads:
        opt.grad.copy_(g)
        opt.step()
    p, m, v = restate_steps(p0, [g.numpy() for g in grads], hooks, 3e-3, wd)
    assert np.allclose(opt.flat.detach().numpy(), p, rtol=1e-5, atol=1e-7)
    assert np.allclose(opt.m.numpy(), m, rtol=1e-5, atol=1e-7 * max(1.0, np.abs(m).max()))
    assert np.allclose(opt.v.numpy(), v, rtol=1e-5, atol=1e-7 * max(1.0, np.abs(v).max()))
    # the hooks changed the trajectory (or, clip alone at a zero gradient aside, would have)
    plain, _, _ = restate_steps(p0, [g.numpy() for g in grads], [], 3e-3, wd)
    assert not np.allclose(p, plain, rtol=1e-6, atol=1e-9)


def test_clip_scale_applied_to_the_whole_gradient():
    """With beta1 = 0 the first moment is the hooked gradient itself: its norm is the threshold."""
    opt = FlatAdam(_model(), alpha=1e-3, beta1=0.0)
    opt.add_hook(GradientClipping(2.5))
    opt.grad.copy_(_grads(opt.flat.numel(), 1)[0])
    g = opt.grad.clone()
    opt.step()
    assert abs(float(torch.linalg.vector_norm(opt.m)) - 2.5) < 1e-5
    assert torch.allclose(opt.m / opt.m.norm(), g / g.norm(), rtol=1e-5, atol=1e-7)
    assert torch.equal(opt.grad, g)                          # the hooks leave opt.grad alone


def test_weight_decay_hook_is_not_adams_decoupled_rate():
    hooks = [("decay", 1e-2)]
    model = _model()
    p0 = FlatAdam(model).flat.detach().clone().numpy()
    grads = [g.numpy() for g in _grads(p0.size)]
    coupled, _, _ = restate_steps(p0, grads, hooks, 1e-3, 0.0)
    decoupled, _, _ = restate_steps(p0, grads, [], 1e-3, 1e-2)
    assert not np.allclose(coupled, decoupled, rtol=1e-4, atol=1e-6)


def test_add_hook_rules():
    opt = FlatAdam(_model())
    opt.add_hook(GradientClipping(1.0))
    opt.add_hook(WeightDecay(1e-3))
    with pytest.raises(ValueError):
        opt.add_hook(GradientClipping(2.0))                  # one hook per kind, whatever its name
    with pytest.raises(ValueError):
        opt.add_hook(WeightDecay(1e-4), name="another")
    with pytest.raises(KeyError):
        opt.add_hook(Lasso(1e-3), name="WeightDecay")        # a name is used once
    with pytest.raises(TypeError):
        opt.add_hook(lambda o: None)
    opt.add_hook(Lasso(1e-3), name="l1")
    assert list(opt._hooks) == ["GradientClipping", "WeightDecay", "l1"]
    assert opt.hook_order() == 1 | (2 << 2) | (3 << 4)
    opt.remove_hook("WeightDecay")
    assert opt.hook_order() == 1 | (3 << 2)
    with pytest.raises(KeyError):
        opt.remove_hook("WeightDecay")


def test_remove_hook_restores_the_plain_rule():
    ma, mb = _model(), _model()
    oa, ob = FlatAdam(ma, alpha=1e-2), FlatAdam(mb, alpha=1e-2)
    for h in (WeightDecay(1e-1), GradientClipping(0.1), Lasso(1e-1)):
        ob.add_hook(h)
    for name in ("WeightDecay", "GradientClipping", "Lasso"):
        ob.remove_hook(name)
    assert ob.hook_order() == 0
    for g in _grads(oa.flat.numel()):
        oa.grad.copy_(g); ob.grad.copy_(g)
        oa.step(); ob.step()
    assert torch.equal(oa.flat, ob.flat) and torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v)


# ---- two gloo ranks with clipping (the pattern of tests/test_dp.py) ----
def _data():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 16, generator=g)
    t = (torch.rand(64, 1, generator=g) < 0.3).int()
    return x, t


def _add_hooks(opt):
    opt.add_hook(GradientClipping(0.05))                     # well below the gradient norm of this model: it bites
    opt.add_hook(WeightDecay(5e-4))
    opt.add_hook(Lasso(1e-4))


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x, t = _data()
        model = _model()
        opt = FlatAdam(model, alpha=1e-2)
        _add_hooks(opt)
        opt.broadcast_parameters(0)
        sl = shard(64, rank, world)
        norms = []
        for _ in range(3):
            opt.zero_grad()
            sigmoid_cross_entropy(model(x[sl]), t[sl]).backward()
            opt.all_reduce_grads()
            norms.append(float(opt.grad.norm()))
            opt.step()
        out[rank] = (opt.flat.detach().clone().numpy(), norms)
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_with_clipping_matches_one_rank():
    world = 2
    port = 33500 + (os.getpid() % 2000)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    p0, n0 = out[0]
    p1, _ = out[1]
    assert np.array_equal(p0, p1)                            # bit-identical ranks
    assert min(n0) > 0.05                                    # the clip was active on every step

    x, t = _data()
    model = _model()
    ref = FlatAdam(model, alpha=1e-2)
    _add_hooks(ref)
    for _ in range(3):                                       # one rank, the whole batch of 64
        ref.zero_grad()
        sigmoid_cross_entropy(model(x), t).backward()
        ref.step()
    assert np.allclose(p0, ref.flat.detach().numpy(), rtol=1e-5, atol=1e-7)
