"""Times the d = 32 fuse-gate and simple-gate GGNN step on TILE-TABLE batches: forward plus backward (weight gradients included)
as the table kernels (csrc/bmp_gate_small_table.hip) and as the composed existing operators (``gate_step(..., fused=False)``, what a
table batch ran before the table kernels existed), in the same process on the same batch object: 1024 pairs of the DDI-shaped
synthetic store in (a) the encoder layout and (b) the encoder layout with de-duplication, 8 untied steps' worth of distinct
message weights (RECORD.txt:404-405).  Four runs of 100 alternating calls after 10, medians with min and p90, by torch.cuda.Event.

The adoption rule is the project's (README, ggnn_dev paragraph): a kind goes to the table kernels by default
(Fn.GATE_TABLE_DEFAULT) if the gain of the median exceeds the two forms' p90 - median spreads together in at least three of the
four runs, in both layouts.

Report only: ``predict`` pairs/s of the recorded model (FuseGGNN(16, 32, 8, weight_tying=False) + HolE, eval()) at 1024 pairs on
the per-instance packed batch and on the de-duplicated encoder layout (collated beforehand), and ms per replay of
GraphedTrainStep at 32 pairs for GateGGNN with the table kernels and with the switch off (the composed chain a static batch ran
before).

The driver opens no GPU itself: every leg -- the step timing, the predict rates, the replay timing -- is a child process under a
time limit of its own (tools/table_probe_lib.py), and the first leg that fails or runs out of time ends the probe.  One JSON line
per run, then one summary line.
python tools/gate_table_probe.py [--runs 4] [--out FILE]          (profiles/gate_table_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
import table_probe_lib as T                                    # noqa: E402

D, LAYERS = 32, 8
KINDS = {"fuse": 0, "gate": 1}
# the step leg makes 6 alternating timings per run (2 layouts x fuse, fuse with masks, gate), 24 in four runs, of 8 steps each
# where the newer probes' legs time 4 layers: 24 x 2 x T.PAIR_SECONDS; the predict leg is three times 35 calls: a replay leg's limit
LEG_SECONDS = {"steps": 24 * 2 * T.PAIR_SECONDS, "predict": T.REPLAY_SECONDS, "replay": T.REPLAY_SECONDS}


def step_run(Fn, pb, dev):
    import torch
    N = pb.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    x = f(N, D).requires_grad_()
    dout = f(N, D)
    keep = (torch.rand(N, D, device=dev) >= 0.05).float() / 0.95
    r = {}
    for kname, kind in KINDS.items():
        nu = (3 if kind == 0 else 1) * D
        W = [[f(4 * D, D).requires_grad_(), f(4, D).requires_grad_(), f(2 * D, nu).requires_grad_(), f(nu).requires_grad_()]
             for _ in range(LAYERS)]

        def step(l, fused, k):
            w = W[l]
            out = Fn.gate_step(x, w[0], w[1], w[2], w[3], kind, k, pb, fused)
            torch.autograd.grad(out, [x] + w, dout)

        for k, tag in ((None, ""), (keep, "_keep")) if kind == 0 else ((None, ""),):
            r[f"{kname}{tag}"] = T.table_against_composed(Fn.GATE_PATHS, lambda l, fused: step(l, fused, k), LAYERS)
    return r


def leg_steps(runs):
    """One JSON line per run: the step of both kinds in both table layouts."""
    from bmp import functional as Fn
    dev, ds, i1, i2, _lab = T.world()
    batches = T.table_batches(ds, i1, i2)
    Fn.GATE_TABLE_DEFAULT.update(fuse=True, gate=True)          # "table" means the kernels here, whatever the default says
    for run in range(runs):
        res = dict(run=run, pairs=T.B, d=D, layers=LAYERS)
        for name, eb in batches.items():
            res[name] = dict(rows=eb.pb_enc.n_rows, tiles=eb.pb_enc.n_mtiles, **step_run(Fn, eb.pb_enc, dev))
        print(json.dumps(res), flush=True)


def predict_rate(model, batch, reps=30):
    import numpy as np
    import torch
    for _ in range(5):
        model.predict(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); model.predict(batch); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return T.B / float(np.median(ts))


def leg_predict():
    """One JSON line: the recorded model's ``predict`` pairs/s per instance, on the de-duplicated table batch and there with
    the switch off."""
    import torch
    from bmp import functional as Fn, packed
    from bmp.ggnn_gate import FuseGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    dev, ds, i1, i2, _lab = T.world()
    eb = T.table_batches(ds, i1, i2)["encoder_dedup"]
    Fn.GATE_TABLE_DEFAULT.update(fuse=True, gate=True)
    torch.manual_seed(0)
    model = GraphConvPredictorForPair(FuseGGNN(16, D, LAYERS, weight_tying=False), None, build_link_predictor("hole", 16, 1)).to(dev).eval()
    pb = packed.pack_from_store_device(ds, [i1, i2])
    res = dict(per_instance=predict_rate(model, pb), encoder_dedup=predict_rate(model, eb))
    Fn.GATE_TABLE_DEFAULT.update(fuse=False, gate=False)
    res["encoder_dedup_composed"] = predict_rate(model, eb)
    print(json.dumps(dict(predict_pairs_per_s=res)), flush=True)


def leg_replay():
    """One JSON line: ms per replay of the recorded GateGGNN training step at 32 pairs, with the switch off and on."""
    import torch
    from bmp import functional as Fn
    from bmp.ggnn_gate import GateGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    dev, ds, i1, i2, lab = T.world()
    res = {}
    for table in (False, True):
        Fn.GATE_TABLE_DEFAULT.update(fuse=table, gate=table)
        torch.manual_seed(1)
        model = GraphConvPredictorForPair(GateGGNN(16, D, LAYERS, weight_tying=False), None, build_link_predictor("hole", 16, 1)).to(dev)
        res["table" if table else "composed"] = T.replay_ms(Fn.GATE_PATHS, ds, i1, i2, lab, model, table)
    print(json.dumps(dict(replay32_gate=res)), flush=True)


def main():
    runs = int(T.arg("--runs", 4))
    if T.arg("--leg"):
        return {"steps": lambda: leg_steps(runs), "predict": leg_predict, "replay": leg_replay}[T.arg("--leg")]()
    got = T.run_legs(__file__, [(leg, D, LEG_SECONDS[leg]) for leg in ("steps", "predict", "replay")], runs, quiet=("predict", "replay"))
    if got is None:
        return 1
    lines = [l for l in got if "run" in l]
    layouts = ("encoder", "encoder_dedup")
    passes = lambda key: [sum(l[lay][key]["passes"] for l in lines) for lay in layouts]
    need = 3 if runs >= 4 else runs
    adopt = dict(fuse=bool(min(passes("fuse") + passes("fuse_keep")) >= need), gate=bool(min(passes("gate")) >= need))
    summary = dict(summary=True, runs=runs, passes={k: dict(zip(layouts, passes(k))) for k in ("fuse", "fuse_keep", "gate")}, adopt=adopt)
    for l in got:                                        # report only: the recorded model's predict, the recorded step at 32 pairs
        if "run" not in l:
            summary.update(l)
    T.finish(lines, summary)
    return 0


if __name__ == "__main__":
    sys.exit(main())
