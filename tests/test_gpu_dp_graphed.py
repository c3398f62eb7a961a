"""The recorded training step (bmp.dp.GraphedTrainStep) with more than one rank: two ranks (gloo collectives, both on cuda:0 --
one MI355X is all a test box has; RCCL on two GPUs where the box has them) record the step as two graphs, replay the first,
all-reduce the flat gradient eagerly and replay the update.  Ranks must stay bit-identical, never issue a collective while a
recording is open, and equal one process that restates the data-parallel step on the two shards: the mean of the shard
gradients with contiguous shares, or Chainer's ParallelUpdater (strided shares ``batch[r::2]``, summed gradients)."""
import os
import socket
import time
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from parity_util import close              # noqa: E402

B, WORLD, STEPS = 16, 2, 8                 # pairs per rank, ranks, global batches

CFGS = {
    "d64": dict(hidden_dim=64, out_dim=32, n_layers=2, attn="nie", head=4),
    "ref_ntn": dict(hidden_dim=32, out_dim=16, n_layers=8, attn="nie", weight_tying=False, sim_method="ntn", mlp_hidden=()),
}
# GradientClipping thresholds between the norms of the mean and of the sum of the two shards' gradients on these batches
# (d64: 0.15-0.65 and 0.3-1.3; ref_ntn: 0.3-1.4 and 0.6-2.9): the clip binds on the sum in most steps, on the mean in few,
# so the hooks tell the two reductions apart
CLIP = {"d64": 0.3, "ref_ntn": 0.8}


# ---- shared by the ranks and the single-process restatement ------------------------------------------------------------
def _data(dev):
    from bmp import packed, synth
    store = synth.make_store(60, seed=3, n_lo=3, n_hi=100, n_mean=20)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev)
    rs = np.random.RandomState(8)
    n = STEPS * B * WORLD
    i1, i2 = rs.randint(0, 60, n), rs.randint(0, 60, n)
    lab = (rs.uniform(size=(n, 1)) < 0.35).astype(np.int32)
    lab[::17] = -1
    return ds, i1, i2, lab


def _model(cfg, dev):
    from bmp.predictor import build_pair_predictor
    torch.manual_seed(5)
    return build_pair_predictor(**CFGS[cfg]).to(dev)


def _opt(model, cfg, hooks, grad_reduce="mean"):
    from bmp.dp import FlatAdam, GradientClipping, WeightDecay
    opt = FlatAdam(model, alpha=1e-3, grad_reduce=grad_reduce)
    if hooks:                                           # in train_binary.py's order (538-543)
        opt.add_hook(GradientClipping(CLIP[cfg]))
        opt.add_hook(WeightDecay(1e-2))
    return opt


def _shares(k, share):
    g = np.arange(k * B * WORLD, (k + 1) * B * WORLD)
    return [g[r * B:(r + 1) * B] for r in range(WORLD)] if share == "contiguous" else [g[r::WORLD] for r in range(WORLD)]


# ---- the ranks ------------------------------------------------------------------------------------------------------------
def _guard_collectives():
    """dist.all_reduce refuses to run while the current stream records a graph; counts the calls it lets through."""
    calls = [0]
    orig = dist.all_reduce

    def all_reduce(*a, **k):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dist.all_reduce issued while a graph is being recorded")
        calls[0] += 1
        return orig(*a, **k)

    dist.all_reduce = all_reduce
    return calls


def _run_static(dev, rank, cfg, hooks, share, grad_reduce):
    from bmp.dp import GraphedTrainStep
    from bmp.trainer import PairBatches
    calls = _guard_collectives()
    ds, i1, i2, lab = _data(dev)
    model = _model(cfg, dev)
    opt = _opt(model, cfg, hooks, grad_reduce)
    opt.broadcast_parameters(0)
    batches = PairBatches(ds, i1, i2, lab, B, layout="static", rank=rank, world=WORLD, share=share)
    stepper = GraphedTrainStep(model, opt)
    losses = []
    for sb, _t in batches:
        assert callable(getattr(sb, "emit", None))
        losses.append(float(stepper(sb).detach()))
    assert len(stepper.graphs) == 1 and opt.t == STEPS, (len(stepper.graphs), opt.t)
    assert calls[0] == stepper.warmup + STEPS, calls[0]         # one eager all-reduce per step (and per warm-up step)
    return dict(flat=opt.flat.cpu(), losses=losses)


def _run_packed(dev, rank, cfg):
    from bmp import packed
    from bmp.dp import GraphedTrainStep
    calls = _guard_collectives()
    ds, i1, i2, lab = _data(dev)
    mg, me = _model(cfg, dev), _model(cfg, dev)
    og, oe = _opt(mg, cfg, False), _opt(me, cfg, False)
    og.broadcast_parameters(0); oe.broadcast_parameters(0)
    n_batches = 3

    def batch(k):
        s = _shares(k, "contiguous")[rank]
        return packed.pack_from_store_device(ds, [i1[s], i2[s]], labels=lab[s])

    graphed, eager = [batch(k) for k in range(n_batches)], [batch(k) for k in range(n_batches)]
    stepper = GraphedTrainStep(mg, og)
    lg, le = [], []
    for _rep in range(2):                               # every batch's recording replayed twice
        for (pg, tg), (pe, te) in zip(graphed, eager):
            lg.append(float(stepper(pg, tg).detach()))
            loss = oe.functional_loss(pe, t=te); loss.backward(); oe.collect_grads(); oe.all_reduce_grads(); oe.step()
            le.append(float(loss.detach()))
    assert len(stepper.graphs) == n_batches and og.t == oe.t == 2 * n_batches
    assert calls[0] == n_batches * stepper.warmup + 2 * 2 * n_batches, calls[0]
    return dict(flat=og.flat.cpu(), eager=oe.flat.cpu(), losses=lg, eager_losses=le)


def _run_fit(dev, rank, cfg):
    from bmp.trainer import PairBatches, fit
    _guard_collectives()
    ds, i1, i2, lab = _data(dev)
    n = 3 * B * WORLD + 6                               # three full global batches and a remainder of 3 pairs per rank
    out = {}
    for layout in ("static", "instance"):
        model = _model(cfg, dev)
        opt = _opt(model, cfg, False)
        opt.broadcast_parameters(0)
        batches = PairBatches(ds, i1[:n], i2[:n], lab[:n], B, shuffle=True, seed=2, layout=layout, rank=rank, world=WORLD)
        logs = fit(model, opt, batches, epochs=2)
        assert opt.t == 2 * 4, opt.t
        out[layout] = opt.flat.cpu()
        out[layout + "_loss"] = [log["main/loss"] for log in logs]
    return out


def _worker(rank, port, backend, mode, args, path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=WORLD, timeout=timedelta(seconds=120))
    try:
        run = {"static": _run_static, "packed": _run_packed, "fit": _run_fit}[mode]
        out = run(dev, rank, *args)
        torch.cuda.synchronize()
        torch.save(out, os.path.join(path, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ranks(tmp_path, mode, args, backend="gloo", timeout=400):
    """Both ranks in fresh processes; any non-zero exit fails the test (no retry)."""
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, backend, mode, args, str(tmp_path))) for r in range(WORLD)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + timeout
    for p in procs:
        p.join(timeout=max(1.0, deadline - time.monotonic()))
    hung = [p.pid for p in procs if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert not hung, f"ranks still running after {timeout} s"
    assert [p.exitcode for p in procs] == [0] * WORLD, [p.exitcode for p in procs]
    return [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(WORLD)]


# ---- the single-process restatements ----------------------------------------------------------------------------------
def _restated(cfg, hooks, share, grad_reduce):
    """One process, both shards packed as usual batches, their eager gradients averaged (or summed), one FlatAdam step."""
    from bmp import packed
    dev = torch.device("cuda:0")
    ds, i1, i2, lab = _data(dev)
    model = _model(cfg, dev)
    ref = _opt(model, cfg, hooks)
    losses = [[] for _ in range(WORLD)]
    for k in range(STEPS):
        acc = None
        for r, s in enumerate(_shares(k, share)):
            pb, t = packed.pack_from_store_device(ds, [i1[s], i2[s]], labels=lab[s])
            loss = ref.functional_loss(pb, t=t); loss.backward(); ref.collect_grads()
            acc = ref.grad.clone() if acc is None else acc + ref.grad
            losses[r].append(float(loss.detach()))
        ref.grad = acc / WORLD if grad_reduce == "mean" else acc
        ref.step()
    return ref.flat.cpu(), losses


def _check_static(out, cfg, hooks, share, grad_reduce, what):
    assert torch.equal(out[0]["flat"], out[1]["flat"]), f"{what}: ranks differ"
    want, losses = _restated(cfg, hooks, share, grad_reduce)
    for r in range(WORLD):
        close(torch.tensor(out[r]["losses"]), torch.tensor(losses[r]), f"{what}: rank {r} losses of {STEPS} steps", tol=1e-4)
    close(out[0]["flat"], want, f"{what}: parameters after {STEPS} steps", tol=1e-4)
    assert not np.allclose(out[0]["losses"][0], out[0]["losses"][-1])       # (different batches: the losses move)
    if hooks:
        # the hooks see the reduced gradient: the other reduction lands ten tolerances away or more (measured: 17-25; Adam
        # alone barely tells them apart)
        other, _ = _restated(cfg, hooks, share, "sum" if grad_reduce == "mean" else "mean")
        assert (other - want).abs().max().item() > 1e-3 * want.abs().max().item(), f"{what}: sum and mean indistinguishable"


@pytest.mark.parametrize("hooks", [False, True], ids=["plain", "clip+decay"])
@pytest.mark.parametrize("cfg", ["d64", "ref_ntn"])
def test_static_two_ranks_mean(tmp_path, cfg, hooks):
    out = _ranks(tmp_path, "static", (cfg, hooks, "contiguous", "mean"))
    _check_static(out, cfg, hooks, "contiguous", "mean", f"graphed DP {cfg} hooks={hooks}, mean")


@pytest.mark.parametrize("hooks", [False, True], ids=["plain", "clip+decay"])
@pytest.mark.parametrize("cfg", ["d64", "ref_ntn"])
def test_static_two_ranks_parallel_updater(tmp_path, cfg, hooks):
    out = _ranks(tmp_path, "static", (cfg, hooks, "strided", "sum"))
    _check_static(out, cfg, hooks, "strided", "sum", f"graphed DP {cfg} hooks={hooks}, strided + sum")


def test_packed_two_ranks(tmp_path):
    out = _ranks(tmp_path, "packed", ("d64",))
    assert torch.equal(out[0]["flat"], out[1]["flat"]), "graphed packed DP: ranks differ"
    assert torch.equal(out[0]["eager"], out[1]["eager"])
    for r in range(WORLD):
        close(torch.tensor(out[r]["losses"]), torch.tensor(out[r]["eager_losses"]), f"graphed packed DP: rank {r} losses", tol=1e-4)
    close(out[0]["flat"], out[0]["eager"], "graphed packed DP: parameters against the eager DP step", tol=1e-4)


def test_fit_static_two_ranks(tmp_path):
    out = _ranks(tmp_path, "fit", ("d64",))
    assert torch.equal(out[0]["static"], out[1]["static"]), "fit on static batches: ranks differ"
    assert torch.equal(out[0]["instance"], out[1]["instance"])
    close(out[0]["static"], out[0]["instance"], "fit: static (graphed) against instance (eager) layout, 2 epochs", tol=1e-4)
    for r in range(WORLD):
        close(torch.tensor(out[r]["static_loss"]), torch.tensor(out[r]["instance_loss"]), f"fit: rank {r} main/loss", tol=1e-4)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL between two ranks needs two GPUs")
def test_static_two_ranks_rccl(tmp_path):
    out = _ranks(tmp_path, "static", ("d64", False, "contiguous", "mean"), backend="nccl")
    _check_static(out, "d64", False, "contiguous", "mean", "graphed DP d64 over RCCL")
