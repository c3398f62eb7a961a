"""Times the jumping-knowledge step at d = 64 and 128 on TILE-TABLE batches: forward plus backward (weight gradients included) as
the table kernels (csrc/bmp_jk_table.hip) and as the composed existing operators (``jk_step(..., fused=False)``: MsgFn +
LinearRowsFn, what a table batch ran before the table kernels existed), in the same process on the same batch object: 1024 pairs of
the DDI-shaped synthetic store in (a) the encoder layout and (b) the encoder layout with de-duplication, 4 untied steps' worth of
distinct weights, the jknet update (Nu = d) and the jk_gru update (Nu = 2d, with its self loop) apart.  Four runs of 100
alternating calls after 10, medians with min and p90, by torch.cuda.Event.

The adoption rule is the project's (README, ggnn_dev paragraph): a (kind, width) goes to the table kernels by default
(Fn.JK_TABLE_DEFAULT) if the gain of the median exceeds the two forms' p90 - median spreads together in at least three of the four
runs, in both layouts.

Report only: ms per replay of GraphedTrainStep at 32 pairs for a JKGruGGNN + HolE model with the table kernels and with the switch
off (the composed chain a static batch ran before).

The driver opens no GPU itself: every leg -- the step timing of one width, the replay timing of one width -- is a child process
under a time limit of its own (tools/table_probe_lib.py), and the first leg that fails or runs out of time ends the probe.  One JSON line per run, then one
summary line.
python tools/jk_table_probe.py [--runs 4] [--out FILE]          (profiles/jk_table_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
import table_probe_lib as T                                    # noqa: E402

WIDTHS, LAYERS = (64, 128), 4
KINDS = {"jknet": (1, False), "jk_gru": (2, True)}            # Nu / d, self loop
# (the step leg of one width makes 4 alternating timings per run, 16 in four runs: 300 s since the probe's first profile)
LEG_SECONDS = {"steps": 300, "replay": T.REPLAY_SECONDS}


def step_run(Fn, pb, dev, d, ng, loop):
    import torch
    N = pb.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    x = f(N, d).requires_grad_()
    dout = f(N, ng * d)
    W = [[f(4 * d, d).requires_grad_(), f(4, d).requires_grad_(), f(d, d).requires_grad_() if loop else None,
          f(d).requires_grad_() if loop else None, f(2 * d, ng * d).requires_grad_(), f(ng * d).requires_grad_()] for _ in range(LAYERS)]

    def step(l, fused):
        w = W[l]
        out = Fn.jk_step(x, *w, pb, fused)
        torch.autograd.grad(out, [x] + [t for t in w if t is not None], dout)

    return T.table_against_composed(Fn.JK_PATHS, step, LAYERS)


def leg_steps(d, runs):
    """One JSON line per run: the step of both kinds at width ``d`` in both table layouts."""
    from bmp import functional as Fn
    dev, ds, i1, i2, _lab = T.world()
    batches = T.table_batches(ds, i1, i2)
    Fn.JK_TABLE_DEFAULT.update({k: True for k in Fn.JK_TABLE_DEFAULT})      # "table" means the kernels here, whatever the default says
    for run in range(runs):
        res = dict(run=run, d=d, pairs=T.B, layers=LAYERS)
        for kind, (ng, loop) in KINDS.items():
            for name, eb in batches.items():
                res[f"{kind}_{name}"] = dict(rows=eb.pb_enc.n_rows, tiles=eb.pb_enc.n_mtiles, **step_run(Fn, eb.pb_enc, dev, d, ng, loop))
        print(json.dumps(res), flush=True)


def leg_replay(d):
    """One JSON line: ms per replay of the recorded JKGruGGNN training step at 32 pairs (load + replay, 200 of them after 20),
    with the switch off and on."""
    import torch
    from bmp import functional as Fn
    from bmp.ggnn_jk import JKGruGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    dev, ds, i1, i2, lab = T.world()
    res = dict(replay32_jk_gru=True, d=d)
    for table in (False, True):
        Fn.JK_TABLE_DEFAULT.update({k: table for k in Fn.JK_TABLE_DEFAULT})
        torch.manual_seed(1)
        enc = JKGruGGNN(16, d, LAYERS, weight_tying=False, update_tying=False, self_loop=True)
        model = GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev)
        res["table" if table else "composed"] = T.replay_ms(Fn.JK_PATHS, ds, i1, i2, lab, model, table)
    print(json.dumps(res), flush=True)


def main():
    runs = int(T.arg("--runs", 4))
    if T.arg("--leg"):
        return leg_steps(int(T.arg("--d")), runs) if T.arg("--leg") == "steps" else leg_replay(int(T.arg("--d")))
    lines = T.run_legs(__file__, [(leg, d, LEG_SECONDS[leg]) for leg in ("steps", "replay") for d in WIDTHS], runs)
    if lines is None:
        return 1
    need = 3 if runs >= 4 else runs
    layouts = ("encoder", "encoder_dedup")
    steps = [l for l in lines if "run" in l]
    passes = {f"{kind}_{d}": {name: sum(l[f"{kind}_{name}"]["passes"] for l in steps if l["d"] == d) for name in layouts}
              for kind in KINDS for d in WIDTHS}
    adopt = {k: bool(min(v.values()) >= need) for k, v in passes.items()}
    summary = dict(summary=True, runs=runs, passes=passes, adopt=adopt)
    T.finish(lines, summary)
    return 0


if __name__ == "__main__":
    sys.exit(main())
