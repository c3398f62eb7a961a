"""Chainer's ParallelUpdater semantics as options of the data-parallel plumbing, on the CPU: the strided share of a global
batch (``PairBatches(share="strided")``: device r takes ``batch[r::n]``) and the summed gradient
(``FlatAdam(grad_reduce="sum")``: the per-device gradients of each device's mean loss added up, as ``addgrads`` does).
The defaults stay what they were: the contiguous share and the mean."""
import os
import socket
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from bmp.dp import FlatAdam, GradientClipping, WeightDecay
from bmp.mlp import MLP
from bmp.predictor import sigmoid_cross_entropy
from bmp.trainer import PairBatches


def _batches(world, rank, share, n=103, B=8, shuffle=True):
    idx = np.arange(n)
    pb = PairBatches(None, idx, idx, np.zeros((n, 1), np.int32), B, shuffle=shuffle, seed=4, rank=rank, world=world,
                     **({} if share is None else dict(share=share)))
    return list(pb.selections())


def _global(n=103, B=8, world=3, shuffle=True):
    order = np.random.RandomState(4).permutation(n) if shuffle else np.arange(n)
    return [order[lo:lo + B * world] for lo in range(0, n, B * world) if len(order[lo:lo + B * world]) >= world]


@pytest.mark.parametrize("world", [2, 3])
def test_strided_share_is_every_world_th_pair(world):
    glob = _global(world=world)
    per_rank = [_batches(world, r, "strided") for r in range(world)]
    for r in range(world):
        assert len(per_rank[r]) == len(glob)
        for sel, g in zip(per_rank[r], glob):
            assert np.array_equal(sel, g[r::world])
    for k, g in enumerate(glob):
        got = np.concatenate([per_rank[r][k] for r in range(world)])
        assert len(got) == len(g) and np.array_equal(np.sort(got), np.sort(g))       # each pair of the batch once
        if len(g) == 8 * world:
            assert all(len(per_rank[r][k]) == 8 for r in range(world))             # a full batch: batch_size per rank


@pytest.mark.parametrize("world", [2, 3])
def test_contiguous_share_is_unchanged(world):
    glob = _global(world=world)
    for r in range(world):
        default, named = _batches(world, r, None), _batches(world, r, "contiguous")
        assert len(default) == len(named) == len(glob)
        for a, b, g in zip(default, named, glob):
            q, rem = divmod(len(g), world)
            lo = r * q + min(r, rem)
            assert np.array_equal(a, g[lo:lo + q + (1 if r < rem else 0)]) and np.array_equal(a, b)


def test_bad_values_are_refused():
    idx = np.arange(4)
    with pytest.raises(ValueError):
        PairBatches(None, idx, idx, np.zeros((4, 1), np.int32), 2, share="interleaved")
    with pytest.raises(ValueError):
        FlatAdam(MLP(1, (4,), in_dim=3), grad_reduce="avg")
    with pytest.raises(ValueError):
        FlatAdam(MLP(1, (4,), in_dim=3), grad_reduce=None)
    assert FlatAdam(MLP(1, (4,), in_dim=3)).grad_reduce == "mean"


def _data():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 16, generator=g)
    t = (torch.rand(64, 1, generator=g) < 0.3).int()
    return x, t


def _model():
    torch.manual_seed(5)
    return MLP(1, (8, 4), in_dim=16)


def _opt(model, reduce):
    opt = FlatAdam(model, alpha=1e-2, grad_reduce=reduce)
    opt.add_hook(WeightDecay(1e-2))                   # the hooks see the summed gradient: decay against twice the mean,
    opt.add_hook(GradientClipping(0.05))              # then a threshold it crosses
    return opt


def _worker(rank, world, port, path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        x, t = _data()
        model = _model()
        opt = _opt(model, "sum")
        opt.broadcast_parameters(0)
        for _ in range(3):
            opt.zero_grad()
            sigmoid_cross_entropy(model(x[rank::world]), t[rank::world]).backward()
            opt.all_reduce_grads()
            opt.step()
        np.save(os.path.join(path, f"rank{rank}.npy"), opt.flat.detach().numpy())
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_gloo_sum_matches_summed_shards(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert [p.exitcode for p in procs] == [0] * world
    p0, p1 = (np.load(tmp_path / f"rank{r}.npy") for r in range(world))
    assert np.array_equal(p0, p1)                                     # bit-identical across ranks

    # ParallelUpdater restated in one process: strided shards, gradients summed, one update per step
    x, t = _data()
    model = _model()
    ref = _opt(model, "mean")                         # (world 1: the reduction setting does nothing here)
    for _ in range(3):
        acc = torch.zeros_like(ref.grad)
        for r in range(world):
            ref.zero_grad()
            sigmoid_cross_entropy(model(x[r::world]), t[r::world]).backward()
            acc += ref.grad
        ref.grad.copy_(acc)
        ref.step()
    want = ref.flat.detach().numpy()
    assert np.allclose(p0, want, rtol=1e-5, atol=1e-7)

    # and it is not the mean: the same run with the gradients averaged lands elsewhere
    model = _model()
    mean = _opt(model, "mean")
    for _ in range(3):
        acc = torch.zeros_like(mean.grad)
        for r in range(world):
            mean.zero_grad()
            sigmoid_cross_entropy(model(x[r::world]), t[r::world]).backward()
            acc += mean.grad
        mean.grad.copy_(acc / world)
        mean.step()
    assert not np.allclose(p0, mean.flat.detach().numpy(), rtol=1e-5, atol=1e-7)
