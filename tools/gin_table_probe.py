"""Times the GIN layer at d = 64 and 128 on TILE-TABLE batches: forward plus backward (weight gradients included) as the table
kernels (csrc/bmp_gin_table.hip) and as the composed existing operators (``gin_layer(..., fused=False)``: MsgFn + LinearRowsFn,
what a table batch ran before the table kernels existed), in the same process on the same batch object: 1024 pairs of the
DDI-shaped synthetic store in (a) the encoder layout and (b) the encoder layout with de-duplication, 4 untied layers' worth of
distinct weights.  Four runs of 100 alternating calls after 10, medians with min and p90, by torch.cuda.Event.

The adoption rule is the project's (README, ggnn_dev paragraph): a width goes to the table kernels by default
(Fn.GIN_TABLE_DEFAULT) if the gain of the median exceeds the two forms' p90 - median spreads together in at least three of the
four runs, in both layouts.

Report only: ms per replay of GraphedTrainStep at 32 pairs for a four-layer untied GIN + HolE model at d = 64 with the table
kernels and with the switch off (the composed chain a static batch ran before).

The driver opens no GPU itself: every leg -- the layer timing of one width, the replay timing -- is a child process under a time
limit of its own, and the first leg that fails or runs out of time ends the probe.  One JSON line per run, then one summary line.
python tools/gin_table_probe.py [--runs 4] [--out FILE]          (profiles/gin_table_probe.json)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]

WIDTHS, LAYERS, B, REPLAY_D = (64, 128), 4, 1024, 64
LEG_SECONDS = {"layers": 240, "replay": 180}


def layer_run(Fn, pb, dev, d):
    import torch
    from gate_probe import timed_pair
    N = pb.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    x = f(N, d).requires_grad_()
    dout = f(N, d)
    W = [[f(d, d).requires_grad_(), f(d).requires_grad_(), f(d, d).requires_grad_(), f(d).requires_grad_()] for _ in range(LAYERS)]

    def layer(l, fused):
        w = W[l]
        out = Fn.gin_layer(x, *w, None, pb, fused)
        torch.autograd.grad(out, [x] + w, dout)

    before = dict(Fn.GIN_PATHS)
    tf, tc = timed_pair(lambda: [layer(l, True) for l in range(LAYERS)], lambda: [layer(l, False) for l in range(LAYERS)])
    took = {a: Fn.GIN_PATHS[a] - before[a] for a in before}
    assert took["fused"] == took["composed"] == 110 * LAYERS, took          # the two forms really ran
    tf, tc = ({a: b / LAYERS for a, b in t.items()} for t in (tf, tc))
    gain = tc["median_us"] - tf["median_us"]
    spread = (tf["p90_us"] - tf["median_us"]) + (tc["p90_us"] - tc["median_us"])
    return dict(table=tf, composed=tc, gain_us=gain, spreads_us=spread, passes=bool(gain > spread))


def _world():
    import torch
    from bmp import packed, synth
    dev = torch.device("cuda:0")
    store = synth.make_store(544, seed=2018)
    i1, i2, lab = synth.make_pairs(544, seed=777, limit=B)
    return dev, packed.DeviceMolStore(packed.MolStore(store), dev), i1, i2, lab.reshape(-1, 1)


def leg_layers(d, runs):
    """One JSON line per run: the layer at width ``d`` in both table layouts."""
    from bmp import enclayout, functional as Fn
    dev, ds, i1, i2, _lab = _world()
    batches = {"encoder": enclayout.encode_from_store_device(ds, [i1, i2]),
               "encoder_dedup": enclayout.encode_from_store_device(ds, [i1, i2], dedup=True)}
    Fn.GIN_TABLE_DEFAULT.update({k: True for k in Fn.GIN_TABLE_DEFAULT})    # "table" means the kernels here, whatever the default says
    for run in range(runs):
        res = dict(run=run, d=d, pairs=B, layers=LAYERS)
        for name, eb in batches.items():
            assert Fn.gin_table_ok(eb.pb_enc, d)
            res[name] = dict(rows=eb.pb_enc.n_rows, tiles=eb.pb_enc.n_mtiles, **layer_run(Fn, eb.pb_enc, dev, d))
        print(json.dumps(res), flush=True)


def leg_replay(d):
    """One JSON line: ms per replay of the recorded GIN training step at 32 pairs (load + replay, 200 of them after 20), with
    the switch off and on."""
    import numpy as np
    import torch
    from bmp import functional as Fn, packed
    from bmp.dp import FlatAdam, GraphedTrainStep
    from bmp.gin import GIN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    dev, ds, i1, i2, lab = _world()
    res = dict(replay32_gin=True, d=d, layers=LAYERS)
    for table in (False, True):
        Fn.GIN_TABLE_DEFAULT.update({k: table for k in Fn.GIN_TABLE_DEFAULT})
        torch.manual_seed(1)
        enc = GIN(16, d, LAYERS, dropout_ratio=0.0, weight_tying=False)
        model = GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev)
        opt = FlatAdam(model, alpha=1e-3)
        sb = packed.StaticPairBatch(ds, 32)
        stepper = GraphedTrainStep(model, opt)
        before = dict(Fn.GIN_PATHS)
        ts = []
        for k in range(220):
            sl = slice(32 * (k % 32), 32 * (k % 32) + 32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sb.load([i1[sl], i2[sl]], lab[sl]); stepper(sb); torch.cuda.synchronize()
            if k >= 20:
                ts.append((time.perf_counter() - t0) * 1e3)
        took = {a: Fn.GIN_PATHS[a] - before[a] for a in before}
        assert (took["composed"] == 0) == table and (took["fused"] == 0) != table, (table, took)      # what was recorded
        res["table" if table else "composed"] = dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)),
                                                     p90_ms=float(np.percentile(ts, 90)))
    print(json.dumps(res), flush=True)


def _child(leg, d, runs):
    """Runs one leg as a process of its own under its time limit; its JSON lines, or None where it failed or ran out of time."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--d", str(d), "--runs", str(runs)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_SECONDS[leg])
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(error=f"leg {leg} d={d}: no end within {LEG_SECONDS[leg]} s")), flush=True)
        return None
    if r.returncode != 0:
        print(json.dumps(dict(error=f"leg {leg} d={d}: exit status {r.returncode}", tail=r.stderr[-1500:])), flush=True)
        return None
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def main():
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 4
    if "--leg" in sys.argv:
        leg, d = sys.argv[sys.argv.index("--leg") + 1], int(sys.argv[sys.argv.index("--d") + 1])
        return leg_layers(d, runs) if leg == "layers" else leg_replay(d)
    lines = []
    for leg, d in [("layers", w) for w in WIDTHS] + [("replay", REPLAY_D)]:
        got = _child(leg, d, runs)
        if got is None:
            return 1                                     # nothing more is started on the card behind a failed leg
        for l in got:
            print(json.dumps(l), flush=True)
        lines += got
    need = 3 if runs >= 4 else runs
    layouts = ("encoder", "encoder_dedup")
    layers = [l for l in lines if "run" in l]
    passes = {str(d): {name: sum(l[name]["passes"] for l in layers if l["d"] == d) for name in layouts} for d in WIDTHS}
    adopt = {k: bool(min(v.values()) >= need) for k, v in passes.items()}
    summary = dict(summary=True, runs=runs, passes=passes, adopt=adopt)
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            for l in lines:
                fh.write(json.dumps(l) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
