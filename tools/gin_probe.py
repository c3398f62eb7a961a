"""Times one GIN layer, forward plus backward (weight gradients included), as the fused tile kernels (csrc/bmp_gin.hip) and as
the composed existing operators (message operator with W1 for every bond type + row linear), in the same process on the same
batch: 1024 pairs of the DDI-shaped synthetic store, 4 untied layers' worth of distinct weights, d = 128 (and d = 64).  Also the
bare kernel launches of the fused form.  Medians over repeated calls after a warm-up, with the spread, by torch.cuda.Event.
Prints one JSON line.  python tools/gin_probe.py [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd")]
from bmp import functional as Fn, packed, synth, _lib          # noqa: E402
from bmp._lib import check, ptr, stream                        # noqa: E402


def timed(fn, warm=5, reps=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return dict(median_us=float(np.median(ts)), min_us=float(ts.min()), p90_us=float(np.percentile(ts, 90)))


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
        f = lambda *s: torch.randn(*s, device=dev) * 0.1
        x = f(N, d).requires_grad_()
        dout = f(N, d)
        W = [[f(d, d).requires_grad_(), f(d).requires_grad_(), f(d, d).requires_grad_(), f(d).requires_grad_()] for _ in range(layers)]
        keep = (torch.rand(N, d, device=dev) >= 0.5).float() * 2.0

        def layer(l, fused, k):
            w = W[l]
            out = Fn.gin_layer(x, w[0].t(), w[1], w[2].t(), w[3], k, pb, fused)
            torch.autograd.grad(out, [x] + w, dout)

        r = {}
        for fused in (True, False):
            for k, tag in ((None, ""), (keep, "_keep")):
                # the four untied layers in turn (each with its own weights), reported per layer
                t = timed(lambda: [layer(l, fused, k) for l in range(layers)])
                r[("fused" if fused else "composed") + tag + "_fwd_bwd_per_layer"] = {a: b / layers for a, b in t.items()}
        # the bare fused launches
        w = [t.detach() for t in W[0]]
        W1p, W2p, W2np, W1np = Fn.pack_k4(w[0].t()), Fn.pack_k4(w[2].t()), Fn.pack_k4(w[2]), Fn.pack_k4(w[0])
        s, t_, out, dp2, dp1, dh = (torch.empty(N, d, device=dev) for _ in range(6))
        xd = x.detach()
        r["gin_layer_tile_fwd"] = timed(lambda: check(L.bmp_gin_layer_tile_fwd(
            ptr(xd), pb.n_tiles, d, ptr(pb.csr_ptr), ptr(pb.csr_col), ptr(pb.csr_val), ptr(W1p), ptr(w[1]), ptr(W2p), ptr(w[3]), None,
            ptr(s), ptr(t_), ptr(out), stream()), "fwd"))
        r["gin_layer_tile_bwd"] = timed(lambda: check(L.bmp_gin_layer_tile_bwd(
            ptr(dout), ptr(out), None, ptr(t_), pb.n_tiles, d, ptr(pb.csrT_ptr), ptr(pb.csrT_col), ptr(pb.csrT_val), ptr(W2np), ptr(W1np),
            ptr(dp2), ptr(dp1), ptr(dh), stream()), "bwd"))
        r["linear_wgrad_both"] = timed(lambda: (Fn._linear_wgrad(t_, dp2), Fn._linear_wgrad(s, dp1)))
        res[f"d{d}"] = r
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
