"""Times one step of the GGNN with the edge-network message, forward plus backward (weight gradients included), as the fused tile
kernels (csrc/bmp_edge.hip) and as the composed existing operators (message operator, segment pool, row broadcast, GRU operator),
in the same process on the same batch: 1024 pairs of the DDI-shaped synthetic store, 4 steps' worth of distinct weights (the first step in the
first-call form, three in the later-call form), d = 128 and d = 64.  The two forms alternate, so that a drift of the machine meets
both.  Also the bare kernel launches of the fused form.  Medians over repeated calls after a warm-up, with min and p90, by
torch.cuda.Event.  Prints one JSON line.  python tools/edge_probe.py [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd")]
from bmp import functional as Fn, packed, synth, _lib          # noqa: E402
from bmp._lib import check, ptr, stream                        # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(ts):
    ts = np.array(ts)
    return dict(median_us=float(np.median(ts)), min_us=float(ts.min()), p90_us=float(np.percentile(ts, 90)))


def timed(fns, warm=5, reps=30):
    """Every function of ``fns`` in turn, ``reps`` rounds after ``warm`` rounds: one stats dict per function."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(once(fn))
    return [stats(t) for t in ts]


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B, layers = 1024, 4
    store = synth.make_store(544, seed=2018)
    i1, i2, _ = synth.make_pairs(544, seed=777, limit=B)
    pb = packed.pack_from_store(packed.MolStore(store), [i1, i2], device=dev)
    N = pb.n_rows
    res = dict(rows=N, pairs=B, layers=layers)
    for d in (128, 64):
        f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
        x = f(N, d).requires_grad_()
        dout = f(N, d)
        # per step: WT, BT, AT, UcT, b (BT small: S sums about 40 rows, the pad row with its multiplicity)
        W = [[t.requires_grad_() for t in (f(4 * d, d), f(d, d) * 0.02, f(2 * d, 3 * d), f(d, d), f(3 * d))] for _ in range(layers)]

        def step(l, fused):
            out = Fn.edge_step(x, *W[l], l == 0, pb, fused)
            torch.autograd.grad(out, [x] + W[l], dout, allow_unused=True)          # (the first call does not read UcT)

        r = {}
        # the four steps in turn (each with its own weights), reported per step
        tf, tc = timed([lambda: [step(l, True) for l in range(layers)], lambda: [step(l, False) for l in range(layers)]])
        r["fused_fwd_bwd_per_step"] = {a: b / layers for a, b in tf.items()}
        r["composed_fwd_bwd_per_step"] = {a: b / layers for a, b in tc.items()}
        spread = (tf["p90_us"] - tf["median_us"] + tc["p90_us"] - tc["median_us"]) / layers
        r["gain_us"] = (tc["median_us"] - tf["median_us"]) / layers
        r["spread_us"] = spread
        r["fused_stays"] = bool(r["gain_us"] > spread)
        # the bare fused launches, later-call form
        w = [t.detach() for t in W[1]]
        pk = Fn.pack_k4
        WTp, BTp, ATp, UcTp = pk(w[0]), pk(w[1]), pk(w[2]), pk(w[3])
        Wnp, Bp, Anp, Ucp = pk(w[0].t()), pk(w[1].t()), pk(w[2].t()), pk(w[3].t())
        seg = (ptr(pb.row_w), ptr(Fn._row_mol(pb)), ptr(pb.mol_row0), ptr(pb.mol_nrows), pb.n_mols)
        e = lambda n: torch.empty(N, n, device=dev)
        m, rz, c, hout, dh, gda, rh = e(d), e(2 * d), e(d), e(d), e(d), e(8 * d), e(d)
        xd = x.detach()
        for first in (0, 1):
            tag = "first" if first else "later"
            r[f"step_tile_fwd_{tag}"], r[f"step_tile_bwd_{tag}"] = timed([
                lambda: check(L.bmp_ggnn_edge_step_tile_fwd(
                    ptr(xd), pb.n_tiles, d, first, ptr(pb.csr_ptr), ptr(pb.csr_col), ptr(pb.csr_val), *seg, ptr(WTp), ptr(BTp),
                    ptr(ATp), ptr(UcTp), ptr(w[4]), ptr(m), ptr(rz), ptr(c), ptr(hout), stream()), "fwd"),
                lambda: check(L.bmp_ggnn_edge_step_tile_bwd(
                    ptr(dout), ptr(xd), ptr(rz), ptr(c), pb.n_tiles, d, first, ptr(pb.csrT_ptr), ptr(pb.csrT_col), ptr(pb.csrT_val),
                    *seg, ptr(Wnp), ptr(Bp), ptr(Anp), ptr(Ucp), ptr(dh), ptr(gda), ptr(rh), stream()), "bwd")])
        r["linear_wgrad_all"] = timed([lambda: (Fn._linear_wgrad(xd, gda), Fn._linear_wgrad(m, gda[:, 5 * d:], bias=False),
                                                Fn._linear_wgrad(rh, gda[:, 7 * d:], bias=False))])[0]
        res[f"d{d}"] = r
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
