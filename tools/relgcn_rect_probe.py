"""Times one RelGCN layer of unequal widths -- forward plus backward, weight gradients included -- as the rectangular fused kernels
(csrc/bmp_relgcn_rect.hip: PRelRectLayerFn on prepared weights) and as the unfused operators of the same build (PMsgFn:
bmp_msg_fwd / bmp_msg_bwd), in the same process on the same batch object: 1024 pairs of the DDI-shaped synthetic store (a) per
instance, (b) in the encoder layout and (c) in the encoder layout with de-duplication, adjacency rescaled, act = tanh.  Pairs
(d_in, d_out): (16, 128) and (128, 64) -- the default stack [16, 128, 64] --, (16, 64) and (64, 32).  Four runs of 100
alternating calls after 10, medians with min and p90, by torch.cuda.Event.

The adoption rule is the project's: a pair's Fn.REL_RECT_DEFAULT entry is True only if the gain of the median exceeds the two
forms' p90 - median spreads together in at least three of the four runs, in all three layouts.  Pairs not measured stay False.

Report only: a 1024-pair training step (planned FlatAdam step) of RelGCN(out_channels=64, scale_adj=True) + MLP with every pair
off, every pair on, and only the pairs with d_in >= 64 on, in turn; ms per replay of the recorded 32-pair step, the same three ways.

The driver opens no GPU itself: every leg is a child process under a time limit of its own (tools/table_probe_lib.py), one at a
time, and the first leg that fails or runs out of time ends the probe.  One JSON line per run, then one summary line.
python tools/relgcn_rect_probe.py [--runs 4] [--out FILE]          (profiles/relgcn_rect_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
import table_probe_lib as T                                    # noqa: E402

PAIRS = ((16, 128), (128, 64), (16, 64), (64, 32))
LAYOUTS = ("instance", "encoder", "encoder_dedup")
# (the layer leg of one pair makes 3 alternating timings per run, 12 in four runs)
LEG_SECONDS = {"layer": 12 * T.PAIR_SECONDS, "step": 6 * T.PAIR_SECONDS, "replay": 2 * T.REPLAY_SECONDS}


# the report-only legs' switch settings: every pair off, every pair on, and only the pairs with d_in >= 64 on (the default
# stack then runs 16 -> 128 unfused and 128 -> 64 fused)
SETTINGS = {"off": lambda p: False, "on": lambda p: True, "on_from_64": lambda p: p[0] >= 64}


def _switch(Fn, on):
    pick = SETTINGS[on] if isinstance(on, str) else (lambda p: on)
    Fn.REL_RECT_DEFAULT.update({k: bool(pick(k)) for k in Fn.REL_RECT_DEFAULT})


def timed_round_robin(fns, warm=10, reps=100):
    """table_probe_lib.timed_pair for any number of forms: {name: stats}."""
    import torch
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return {k: T.stats(v) for k, v in ts.items()}


def layer_run(Fn, pbs, dev, d_in, d_out):
    import torch
    N = pbs.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    x, dout = f(N, d_in).requires_grad_(), f(N, d_out)
    WT, bE, WsT, bs = f(4 * d_in, d_out), f(4, d_out), f(d_in, d_out), f(d_out)
    Wnat_p, Ws_p = Fn.rel_rect_pack_bwd(WT, WsT)
    Wf = dict(WTp=Fn.pack_k4(WT), bE=bE, WsTp=Fn.pack_k4(WsT), bs=bs, Wnat_p=Wnat_p, Ws_p=Ws_p)
    Wc = dict(WT=WT, bE=bE, WsT=WsT, bs=bs, Wnat=WT.t().contiguous(), Ws=WsT.t().contiguous())
    e = lambda *s: torch.empty(*s, device=dev)
    Gf = dict(o1=e(d_in, 5 * d_out), dbE=e(4, d_out), cs=e(5 * d_out))
    Gc = dict(dWT=e(4 * d_in, d_out), dbE=e(4, d_out), dWsT=e(d_in, d_out), dbs=e(d_out))
    act = Fn.ACT["tanh"]

    def layer(_l, fused):
        # (the prepared-weight Functions count no path themselves: bmp/relgcn.py does, at its dispatch)
        Fn.REL_PATHS["fused" if fused else "composed"] += 1
        if fused:
            out = Fn.PRelRectLayerFn.apply(x, pbs, Wf, Gf, {}, "c0", act)
        else:
            out = Fn.PMsgFn.apply(x, pbs, Wc, Gc, {}, "c0", act)
        torch.autograd.grad(out, [x], dout)

    return T.table_against_composed(Fn.REL_PATHS, layer, 1)


def leg_layer(pair, runs):
    """One JSON line per run: the layer of one (d_in, d_out) in the three layouts."""
    from bmp import functional as Fn
    from bmp import packed
    from bmp.relgcn import rescale_adj
    d_in, d_out = pair
    dev, ds, i1, i2, _lab = T.world()
    assert Fn.rel_rect_supported(d_in, d_out)
    batches = {"instance": packed.pack_from_store_device(ds, [i1, i2])}
    batches.update({k: eb.pb_enc for k, eb in T.table_batches(ds, i1, i2).items()})
    for run in range(runs):
        res = dict(run=run, d_in=d_in, d_out=d_out, pairs=T.B)
        for name in LAYOUTS:
            pb = batches[name]
            assert not pb.oversized
            res[name] = dict(rows=pb.n_rows, tiles=pb.n_mtiles, **layer_run(Fn, rescale_adj(pb), dev, d_in, d_out))
        print(json.dumps(res), flush=True)


def _model(dev):
    import torch
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.relgcn import RelGCN
    torch.manual_seed(1)
    return GraphConvPredictorForPair(RelGCN(out_channels=64, scale_adj=True), None, build_link_predictor("mlp", 64, 1)).to(dev)


def leg_step(runs):
    """One JSON line per run: the planned 1024-pair training step of the default RelGCN + MLP model under SETTINGS, in turn."""
    import torch
    from bmp import functional as Fn
    from bmp import packed
    from bmp.dp import FlatAdam
    dev, ds, i1, i2, lab = T.world()
    pb, t = packed.pack_from_store_device(ds, [i1, i2], labels=lab)
    opts = {}
    for on in SETTINGS:
        _switch(Fn, on)
        opts[on] = FlatAdam(_model(dev), alpha=1e-3)

    def step(on):
        _switch(Fn, on)
        opt = opts[on]
        loss = opt.functional_loss(pb, t=t)
        loss.backward(); opt.collect_grads(); opt.step()

    for run in range(runs):
        before = dict(Fn.REL_PATHS)
        res = timed_round_robin({on: (lambda on=on: step(on)) for on in SETTINGS})
        tk = {a: Fn.REL_PATHS[a] - before[a] for a in before}
        assert tk["fused"] == tk["composed"] == 330, tk          # 110 steps of two layers: 0, 2 and 1 of them fused
        print(json.dumps(dict(step1024=True, run=run, **res)), flush=True)


def _replay_mixed(Fn, ds, i1, i2, lab, model):
    """table_probe_lib.replay_ms for a recording that holds one fused and one unfused layer."""
    import time
    import numpy as np
    import torch
    from bmp import packed
    from bmp.dp import FlatAdam, GraphedTrainStep
    opt = FlatAdam(model, alpha=1e-3)
    sb = packed.StaticPairBatch(ds, 32)
    stepper = GraphedTrainStep(model, opt)
    before = dict(Fn.REL_PATHS)
    ts = []
    for k in range(220):
        sl = slice(32 * (k % 32), 32 * (k % 32) + 32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sb.load([i1[sl], i2[sl]], lab[sl]); stepper(sb); torch.cuda.synchronize()
        if k >= 20:
            ts.append((time.perf_counter() - t0) * 1e3)
    tk = {a: Fn.REL_PATHS[a] - before[a] for a in before}
    assert tk["fused"] == tk["composed"] > 0, tk
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), p90_ms=float(np.percentile(ts, 90)))


def leg_replay():
    """One JSON line: ms per replay of the recorded 32-pair training step of the same model under SETTINGS."""
    from bmp import functional as Fn
    dev, ds, i1, i2, lab = T.world()
    res = dict(replay32_relgcn=True)
    for on in SETTINGS:
        _switch(Fn, on)
        # ("on_from_64" records one layer of each form: replay_ms's check of what was recorded is for the two pure settings)
        if on == "on_from_64":
            res[on] = _replay_mixed(Fn, ds, i1, i2, lab, _model(dev))
        else:
            res[on] = T.replay_ms(Fn.REL_PATHS, ds, i1, i2, lab, _model(dev), on == "on")
    print(json.dumps(res), flush=True)


def main():
    runs = int(T.arg("--runs", 4))
    leg = T.arg("--leg")
    if leg == "layer":
        return leg_layer(tuple(int(v) for v in T.arg("--d").split("x")), runs)
    if leg == "step":
        return leg_step(runs)
    if leg == "replay":
        return leg_replay()
    legs = [("layer", f"{a}x{b}", LEG_SECONDS["layer"]) for a, b in PAIRS] + [("step", 0, LEG_SECONDS["step"]), ("replay", 0, LEG_SECONDS["replay"])]
    lines = T.run_legs(__file__, legs, runs)
    if lines is None:
        return 1
    need = 3 if runs >= 4 else runs
    layers = [l for l in lines if "d_in" in l]
    passes = {f"{a}x{b}": {name: sum(l[name]["passes"] for l in layers if (l["d_in"], l["d_out"]) == (a, b)) for name in LAYOUTS}
              for a, b in PAIRS}
    # (necessary for a True entry of Fn.REL_RECT_DEFAULT, not sufficient: the report-only step figures are read beside it)
    passes_rule = {k: bool(min(v.values()) >= need) for k, v in passes.items()}
    T.finish(lines, dict(summary=True, runs=runs, passes=passes, passes_rule=passes_rule))
    return 0


if __name__ == "__main__":
    sys.exit(main())
