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
before).  One JSON line per run, then one summary line.
python tools/gate_table_probe.py [--runs 4] [--out FILE]          (profiles/gate_table_probe.json)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
from bmp import enclayout, functional as Fn, packed, synth     # noqa: E402
from gate_probe import timed_pair                              # noqa: E402

D, LAYERS, B = 32, 8, 1024


def step_run(pb, dev):
    N = pb.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    x = f(N, D).requires_grad_()
    dout = f(N, D)
    keep = (torch.rand(N, D, device=dev) >= 0.05).float() / 0.95
    r = {}
    for kind, kname in ((0, "fuse"), (1, "gate")):
        nu = (3 if kind == 0 else 1) * D
        W = [[f(4 * D, D).requires_grad_(), f(4, D).requires_grad_(), f(2 * D, nu).requires_grad_(), f(nu).requires_grad_()]
             for _ in range(LAYERS)]

        def step(l, fused, k):
            w = W[l]
            out = Fn.gate_step(x, w[0], w[1], w[2], w[3], kind, k, pb, fused)
            torch.autograd.grad(out, [x] + w, dout)

        for k, tag in ((None, ""), (keep, "_keep")) if kind == 0 else ((None, ""),):
            before = dict(Fn.GATE_PATHS)
            tf, tc = timed_pair(lambda: [step(l, True, k) for l in range(LAYERS)], lambda: [step(l, False, k) for l in range(LAYERS)])
            took = {a: Fn.GATE_PATHS[a] - before[a] for a in before}
            assert took["fused"] == took["composed"] == 110 * LAYERS, took          # the two forms really ran
            tf, tc = ({a: b / LAYERS for a, b in t.items()} for t in (tf, tc))
            gain = tc["median_us"] - tf["median_us"]
            spread = (tf["p90_us"] - tf["median_us"]) + (tc["p90_us"] - tc["median_us"])
            r[f"{kname}{tag}"] = dict(table=tf, composed=tc, gain_us=gain, spreads_us=spread, passes=bool(gain > spread))
    return r


def predict_rate(model, batch, reps=30):
    for _ in range(5):
        model.predict(batch)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); model.predict(batch); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return B / float(np.median(ts))


def replay_ms(ds, i1, i2, lab, table):
    """ms per replay of the recorded GateGGNN training step at 32 pairs (load + replay, 200 of them after 20)."""
    from bmp.dp import FlatAdam, GraphedTrainStep
    from bmp.ggnn_gate import GateGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    Fn.GATE_TABLE_DEFAULT.update(fuse=table, gate=table)
    torch.manual_seed(1)
    model = GraphConvPredictorForPair(GateGGNN(16, D, LAYERS, weight_tying=False), None, build_link_predictor("hole", 16, 1)).to(ds.device)
    opt = FlatAdam(model, alpha=1e-3)
    sb = packed.StaticPairBatch(ds, 32)
    stepper = GraphedTrainStep(model, opt)
    ts = []
    for k in range(220):
        sl = slice(32 * (k % 32), 32 * (k % 32) + 32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sb.load([i1[sl], i2[sl]], lab[sl]); stepper(sb); torch.cuda.synchronize()
        if k >= 20:
            ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), p90_ms=float(np.percentile(ts, 90)))


def main():
    dev = torch.device("cuda:0")
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 4
    store = synth.make_store(544, seed=2018)
    i1, i2, lab = synth.make_pairs(544, seed=777, limit=B)
    lab = lab.reshape(-1, 1)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev)
    batches = {"encoder": enclayout.encode_from_store_device(ds, [i1, i2]),
               "encoder_dedup": enclayout.encode_from_store_device(ds, [i1, i2], dedup=True)}
    lines = []
    Fn.GATE_TABLE_DEFAULT.update(fuse=True, gate=True)          # "table" means the kernels here, whatever the default says
    for run in range(runs):
        res = dict(run=run, pairs=B, d=D, layers=LAYERS)
        for name, eb in batches.items():
            res[name] = dict(rows=eb.pb_enc.n_rows, tiles=eb.pb_enc.n_mtiles, **step_run(eb.pb_enc, dev))
        lines.append(res)
        print(json.dumps(res), flush=True)
    passes = lambda key: [sum(l[lay][key]["passes"] for l in lines) for lay in batches]
    need = 3 if runs >= 4 else runs
    adopt = dict(fuse=bool(min(passes("fuse") + passes("fuse_keep")) >= need), gate=bool(min(passes("gate")) >= need))
    summary = dict(summary=True, runs=runs, passes={k: dict(zip(batches, passes(k))) for k in ("fuse", "fuse_keep", "gate")}, adopt=adopt)
    # report only: the recorded model's predict, and the recorded step at 32 pairs
    from bmp.ggnn_gate import FuseGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    torch.manual_seed(0)
    model = GraphConvPredictorForPair(FuseGGNN(16, D, LAYERS, weight_tying=False), None, build_link_predictor("hole", 16, 1)).to(dev).eval()
    pb = packed.pack_from_store_device(ds, [i1, i2])
    summary["predict_pairs_per_s"] = dict(per_instance=predict_rate(model, pb), encoder_dedup=predict_rate(model, batches["encoder_dedup"]))
    Fn.GATE_TABLE_DEFAULT.update(fuse=False, gate=False)
    summary["predict_pairs_per_s"]["encoder_dedup_composed"] = predict_rate(model, batches["encoder_dedup"])
    summary["replay32_gate"] = dict(composed=replay_ms(ds, i1, i2, lab, False), table=replay_ms(ds, i1, i2, lab, True))
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            for l in lines:
                fh.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
