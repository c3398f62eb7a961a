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
switch off (the composed chain a static batch ran before).

The driver opens no GPU itself: every leg -- the step timing, the replay timing of one width -- is a child process under a time
limit of its own (tools/table_probe_lib.py), and the first leg that fails or runs out of time ends the probe.  One JSON line per
run, then one summary line.
python tools/loop_table_probe.py [--runs 4] [--out FILE]          (profiles/loop_table_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
import table_probe_lib as T                                    # noqa: E402

WIDTHS, LAYERS = (64, 128), 4
# the step leg makes 8 alternating timings per run (2 widths x 2 layouts x first / later), 32 in four runs
LEG_SECONDS = {"steps": 32 * T.PAIR_SECONDS, "replay": T.REPLAY_SECONDS}


def step_run(Fn, pb, dev, d):
    import torch
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

        r[tag] = T.table_against_composed(Fn.LOOP_PATHS, step, LAYERS)
    return r


def leg_steps(runs):
    """One JSON line per run: the step at both widths in both table layouts."""
    from bmp import functional as Fn
    dev, ds, i1, i2, _lab = T.world()
    batches = T.table_batches(ds, i1, i2)
    Fn.LOOP_TABLE_DEFAULT.update({w: True for w in WIDTHS})     # "table" means the kernels here, whatever the default says
    for run in range(runs):
        res = dict(run=run, pairs=T.B, layers=LAYERS)
        for d in WIDTHS:
            for name, eb in batches.items():
                res[f"d{d}_{name}"] = dict(rows=eb.pb_enc.n_rows, tiles=eb.pb_enc.n_mtiles, **step_run(Fn, eb.pb_enc, dev, d))
        print(json.dumps(res), flush=True)


def leg_replay(d):
    """One JSON line: ms per replay of the recorded SelfLoopGGNN training step at 32 pairs, with the switch off and on."""
    import torch
    from bmp import functional as Fn
    from bmp.ggnn_dev import SelfLoopGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    dev, ds, i1, i2, lab = T.world()
    res = {}
    for table in (False, True):
        Fn.LOOP_TABLE_DEFAULT.update({w: table for w in WIDTHS})
        torch.manual_seed(1)
        model = GraphConvPredictorForPair(SelfLoopGGNN(16, d, LAYERS, weight_tying=False), None, build_link_predictor("hole", 16, 1)).to(dev)
        res["table" if table else "composed"] = T.replay_ms(Fn.LOOP_PATHS, ds, i1, i2, lab, model, table)
    print(json.dumps({f"d{d}": res}), flush=True)


def main():
    runs = int(T.arg("--runs", 4))
    if T.arg("--leg"):
        return leg_steps(runs) if T.arg("--leg") == "steps" else leg_replay(int(T.arg("--d")))
    legs = [("steps", 0, LEG_SECONDS["steps"])] + [("replay", d, LEG_SECONDS["replay"]) for d in WIDTHS]
    got = T.run_legs(__file__, legs, runs, quiet=("replay",))
    if got is None:
        return 1
    lines = [l for l in got if "run" in l]
    need = 3 if runs >= 4 else runs
    passes = {d: {f"{name}_{tag}": sum(l[f"d{d}_{name}"][tag]["passes"] for l in lines) for name in ("encoder", "encoder_dedup")
                  for tag in ("first", "later")} for d in WIDTHS}
    adopt = {d: bool(min(passes[d].values()) >= need) for d in WIDTHS}
    summary = dict(summary=True, runs=runs, passes=passes, adopt=adopt, replay32_self_loop={})
    for l in got:                                        # report only: the recorded step at 32 pairs
        if "run" not in l:
            summary["replay32_self_loop"].update(l)
    T.finish(lines, summary)
    return 0


if __name__ == "__main__":
    sys.exit(main())
