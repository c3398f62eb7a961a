"""Times the self-loop GGNN step at d = 64 and 128 on TILE-TABLE batches: forward plus backward (weight gradients included) as the
table kernels (csrc/bmp_loop_table.hip) and as the composed existing operators (``loop_step(..., fused=False)``, what a table
batch ran before the table kernels existed), in the same process on the same batch object: 1024 pairs of the DDI-shaped synthetic
store in (a) the encoder layout and (b) the encoder layout with de-duplication, 4 untied steps' worth of distinct weights, the
first-call form and the later-call form apart.  Four runs of 100 alternating calls after 10, medians with min and p90, by
torch.cuda.Event.

The adoption rule is the project's (README, ggnn_dev paragraph): a width goes to the table kernels by default
(Fn.LOOP_TABLE_DEFAULT) if the gain of the median exceeds the two forms' p90 - median spreads together in at least three of the
four runs, in both layouts and for both call forms.

Report only: ms per replay of GraphedTrainStep at 32 pairs for a SelfLoopGGNN + HolE model with the table kernels and with the
switch off (the composed chain a static batch ran before).  One JSON line per run, then one summary line.
python tools/loop_table_probe.py [--runs 4] [--out FILE]          (profiles/loop_table_probe.json)"""
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

WIDTHS, LAYERS, B = (64, 128), 4, 1024


def step_run(pb, dev, d):
    N = pb.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    x = f(N, d).requires_grad_()
    dout = f(N, d)
    W = [[f(4 * d, d).requires_grad_(), f(4, d).requires_grad_(), f(d, d).requires_grad_(), f(d).requires_grad_(),
          f(2 * d, 3 * d).requires_grad_(), f(d, d).requires_grad_(), f(3 * d).requires_grad_()] for _ in range(LAYERS)]
    r = {}
    for first, tag in ((True, "first"), (False, "later")):
        def step(l, fused):
            w = W[l]
            out = Fn.loop_step(x, *w, first, pb, fused)
            torch.autograd.grad(out, [x] + w, dout, allow_unused=True)        # (a first call does not read UcT)

        before = dict(Fn.LOOP_PATHS)
        tf, tc = timed_pair(lambda: [step(l, True) for l in range(LAYERS)], lambda: [step(l, False) for l in range(LAYERS)])
        took = {a: Fn.LOOP_PATHS[a] - before[a] for a in before}
        assert took["fused"] == took["composed"] == 110 * LAYERS, took          # the two forms really ran
        tf, tc = ({a: b / LAYERS for a, b in t.items()} for t in (tf, tc))
        gain = tc["median_us"] - tf["median_us"]
        spread = (tf["p90_us"] - tf["median_us"]) + (tc["p90_us"] - tc["median_us"])
        r[tag] = dict(table=tf, composed=tc, gain_us=gain, spreads_us=spread, passes=bool(gain > spread))
    return r


def replay_ms(ds, i1, i2, lab, d, table):
    """ms per replay of the recorded SelfLoopGGNN training step at 32 pairs (load + replay, 200 of them after 20)."""
    from bmp.dp import FlatAdam, GraphedTrainStep
    from bmp.ggnn_dev import SelfLoopGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    Fn.LOOP_TABLE_DEFAULT.update({w: table for w in WIDTHS})
    torch.manual_seed(1)
    model = GraphConvPredictorForPair(SelfLoopGGNN(16, d, LAYERS, weight_tying=False), None, build_link_predictor("hole", 16, 1)).to(ds.device)
    opt = FlatAdam(model, alpha=1e-3)
    sb = packed.StaticPairBatch(ds, 32)
    stepper = GraphedTrainStep(model, opt)
    before = dict(Fn.LOOP_PATHS)
    ts = []
    for k in range(220):
        sl = slice(32 * (k % 32), 32 * (k % 32) + 32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sb.load([i1[sl], i2[sl]], lab[sl]); stepper(sb); torch.cuda.synchronize()
        if k >= 20:
            ts.append((time.perf_counter() - t0) * 1e3)
    took = {a: Fn.LOOP_PATHS[a] - before[a] for a in before}
    assert (took["composed"] == 0) == table and (took["fused"] == 0) != table, (table, took)      # what was recorded
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
    Fn.LOOP_TABLE_DEFAULT.update({w: True for w in WIDTHS})     # "table" means the kernels here, whatever the default says
    for run in range(runs):
        res = dict(run=run, pairs=B, layers=LAYERS)
        for d in WIDTHS:
            for name, eb in batches.items():
                res[f"d{d}_{name}"] = dict(rows=eb.pb_enc.n_rows, tiles=eb.pb_enc.n_mtiles, **step_run(eb.pb_enc, dev, d))
        lines.append(res)
        print(json.dumps(res), flush=True)
    need = 3 if runs >= 4 else runs
    passes = {d: {f"{name}_{tag}": sum(l[f"d{d}_{name}"][tag]["passes"] for l in lines) for name in batches for tag in ("first", "later")}
              for d in WIDTHS}
    adopt = {d: bool(min(passes[d].values()) >= need) for d in WIDTHS}
    summary = dict(summary=True, runs=runs, passes=passes, adopt=adopt)
    # report only: the recorded step at 32 pairs
    summary["replay32_self_loop"] = {f"d{d}": dict(composed=replay_ms(ds, i1, i2, lab, d, False), table=replay_ms(ds, i1, i2, lab, d, True))
                                     for d in WIDTHS}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            for l in lines:
                fh.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
