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
limit of its own (tools/table_probe_lib.py), and the first leg that fails or runs out of time ends the probe.  One JSON line per run, then one summary line.
python tools/gin_table_probe.py [--runs 4] [--out FILE]          (profiles/gin_table_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
import table_probe_lib as T                                    # noqa: E402

WIDTHS, LAYERS, REPLAY_D = (64, 128), 4, 64
# (the layer leg of one width makes 2 alternating timings per run, 8 in four runs)
LEG_SECONDS = {"layers": 8 * T.PAIR_SECONDS, "replay": T.REPLAY_SECONDS}


def layer_run(Fn, pb, dev, d):
    import torch
    N = pb.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    x = f(N, d).requires_grad_()
    dout = f(N, d)
    W = [[f(d, d).requires_grad_(), f(d).requires_grad_(), f(d, d).requires_grad_(), f(d).requires_grad_()] for _ in range(LAYERS)]

    def layer(l, fused):
        w = W[l]
        out = Fn.gin_layer(x, *w, None, pb, fused)
        torch.autograd.grad(out, [x] + w, dout)

    return T.table_against_composed(Fn.GIN_PATHS, layer, LAYERS)


def leg_layers(d, runs):
    """One JSON line per run: the layer at width ``d`` in both table layouts."""
    from bmp import functional as Fn
    dev, ds, i1, i2, _lab = T.world()
    batches = T.table_batches(ds, i1, i2)
    Fn.GIN_TABLE_DEFAULT.update({k: True for k in Fn.GIN_TABLE_DEFAULT})    # "table" means the kernels here, whatever the default says
    for run in range(runs):
        res = dict(run=run, d=d, pairs=T.B, layers=LAYERS)
        for name, eb in batches.items():
            assert Fn.gin_table_ok(eb.pb_enc, d)
            res[name] = dict(rows=eb.pb_enc.n_rows, tiles=eb.pb_enc.n_mtiles, **layer_run(Fn, eb.pb_enc, dev, d))
        print(json.dumps(res), flush=True)


def leg_replay(d):
    """One JSON line: ms per replay of the recorded GIN training step at 32 pairs (load + replay, 200 of them after 20), with
    the switch off and on."""
    import torch
    from bmp import functional as Fn
    from bmp.gin import GIN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    dev, ds, i1, i2, lab = T.world()
    res = dict(replay32_gin=True, d=d, layers=LAYERS)
    for table in (False, True):
        Fn.GIN_TABLE_DEFAULT.update({k: table for k in Fn.GIN_TABLE_DEFAULT})
        torch.manual_seed(1)
        enc = GIN(16, d, LAYERS, dropout_ratio=0.0, weight_tying=False)
        model = GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev)
        res["table" if table else "composed"] = T.replay_ms(Fn.GIN_PATHS, ds, i1, i2, lab, model, table)
    print(json.dumps(res), flush=True)


def main():
    runs = int(T.arg("--runs", 4))
    if T.arg("--leg"):
        return leg_layers(int(T.arg("--d")), runs) if T.arg("--leg") == "layers" else leg_replay(int(T.arg("--d")))
    legs = [("layers", w, LEG_SECONDS["layers"]) for w in WIDTHS] + [("replay", REPLAY_D, LEG_SECONDS["replay"])]
    lines = T.run_legs(__file__, legs, runs)
    if lines is None:
        return 1
    need = 3 if runs >= 4 else runs
    layouts = ("encoder", "encoder_dedup")
    layers = [l for l in lines if "run" in l]
    passes = {str(d): {name: sum(l[name]["passes"] for l in layers if l["d"] == d) for name in layouts} for d in WIDTHS}
    adopt = {k: bool(min(v.values()) >= need) for k, v in passes.items()}
    summary = dict(summary=True, runs=runs, passes=passes, adopt=adopt)
    T.finish(lines, summary)
    return 0


if __name__ == "__main__":
    sys.exit(main())
