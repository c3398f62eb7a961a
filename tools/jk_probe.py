"""Times one step of the jumping-knowledge GGNN encoders -- the GGNN message and the relu-linear update, forward plus backward
(weight gradients included) -- as the fused tile kernels (csrc/bmp_jk.hip) and as the composed existing operators (message
operator + row linear with relu on [h, m]), in the same process on the same batch: 1024 pairs of the DDI-shaped synthetic store,
4 untied steps' worth of distinct weights, d = 128 and d = 64.  Kinds: 'jknet' (Nu = d), 'jk_gru' (Nu = 2d, the layer in front of the
GRU; the GRU itself is the same operator in both forms and is not timed) and, for information, 'jk_gru_loop' (with the self loop).
The fused and the composed form of a step alternate call by call (100 of each after 10 warm-ups), timed by torch.cuda.Event;
--runs of them (4), one JSON line each, then one line with the adoption rule of DESIGN.md 3e per (kind, width): composed
median - fused median must exceed the sum of the two forms' p90 - median spreads in at least three of four runs.
python tools/jk_probe.py [--widths 128,64] [--runs 4] [--out FILE]          (profiles/jk_probe.json)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
from bmp import functional as Fn, packed, synth          # noqa: E402
from table_probe_lib import timed_pair                   # noqa: E402

KINDS = (("jknet", 1, False), ("jk_gru", 2, False), ("jk_gru_loop", 2, True))


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def adopted(runs, key):
    """(wins, per-run margins): a run wins when composed median - fused median > the sum of the two p90 - median spreads."""
    wins, margins = 0, []
    for r in runs:
        f, c = r[key]["fused"], r[key]["composed"]
        gain = c["median_us"] - f["median_us"]
        spread = (c["p90_us"] - c["median_us"]) + (f["p90_us"] - f["median_us"])
        wins += gain > spread
        margins.append(dict(gain_us=gain, spread_us=spread))
    return wins, margins


def main():
    dev = torch.device("cuda:0")
    B, layers = 1024, 4
    widths = [int(w) for w in _arg("--widths", "128,64").split(",")]
    n_runs = int(_arg("--runs", "4"))
    for k in Fn.JK_STEP_DEFAULT:                                 # "fused" means the kernels, whatever the default says
        Fn.JK_STEP_DEFAULT[k] = True
    store = synth.make_store(544, seed=2018)
    i1, i2, _ = synth.make_pairs(544, seed=777, limit=B)
    pb = packed.pack_from_store(packed.MolStore(store), [i1, i2], device=dev)
    N = pb.n_rows
    f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    runs = []
    for run in range(n_runs):
        res = dict(run=run, rows=N, pairs=B, layers=layers)
        for d in widths:
            x = f(N, d).requires_grad_()
            for kname, ng, loop in KINDS:
                nu = ng * d
                dout = f(N, nu)
                W = [[f(4 * d, d).requires_grad_(), f(4, d).requires_grad_()]
                     + ([f(d, d).requires_grad_(), f(d).requires_grad_()] if loop else [None, None])
                     + [f(2 * d, nu).requires_grad_(), f(nu).requires_grad_()] for _ in range(layers)]

                def step(l, fused):
                    w = W[l]
                    out = Fn.jk_step(x, *w, pb, fused)
                    torch.autograd.grad(out, [x] + [t for t in w if t is not None], dout)

                before = dict(Fn.JK_PATHS)
                tf, tc = timed_pair(lambda: [step(l, True) for l in range(layers)], lambda: [step(l, False) for l in range(layers)])
                took = {k: Fn.JK_PATHS[k] - before[k] for k in before}
                assert took["fused"] == took["composed"] == 110 * layers, took
                res[f"{kname}_d{d}"] = dict(fused={a: b / layers for a, b in tf.items()}, composed={a: b / layers for a, b in tc.items()})
        runs.append(res)
        print(json.dumps(res), flush=True)
    summary = dict(rule="composed median - fused median > (composed p90 - median) + (fused p90 - median), in >= 3 of 4 runs", decisions={})
    for d in widths:
        for kname, _, _ in KINDS:
            key = f"{kname}_d{d}"
            wins, margins = adopted(runs, key)
            summary["decisions"][key] = dict(wins=int(wins), runs=n_runs, fused_by_default=bool(wins >= 3), margins=margins)
    print(json.dumps(summary), flush=True)
    if "--out" in sys.argv:
        with open(_arg("--out", None), "w") as fh:
            for r in runs + [summary]:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
