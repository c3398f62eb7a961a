"""Times one step of the fuse-gate and of the simple-gate GGNN, forward plus backward (weight gradients included), as the fused
tile kernels (csrc/bmp_gate.hip) and as the composed existing operators (message operator + row linear on [h, m] + torch
elementwise), in the same process on the same batch: 1024 pairs of the DDI-shaped synthetic store, 4 untied steps' worth of
distinct message weights, d = 128 (and d = 64); and d = 32 (the wave-local kernels of csrc/bmp_gate_small.hip) with 8 untied
steps, the recorded depth (RECORD.txt:404-405).  Also the bare kernel launches of the fused form.  Medians over repeated calls
after a warm-up, with the spread, by torch.cuda.Event; the fused and the composed form of a step alternate call by call (100 of
each after 10).  Prints one JSON line.
python tools/gate_probe.py [--widths 128,64,32] [--out FILE]     (profiles/gate_probe.json: --widths 128,64;
                                                                  profiles/gate_probe_d32.json: --widths 32, four runs, one line each)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
from bmp import functional as Fn, packed, synth, _lib          # noqa: E402
from bmp._lib import check, ptr, stream                        # noqa: E402
from table_probe_lib import stats, timed_pair                  # noqa: E402


def timed(fn, warm=5, reps=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return stats(ts)


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B = 1024
    widths = [int(w) for w in sys.argv[sys.argv.index("--widths") + 1].split(",")] if "--widths" in sys.argv else [128, 64, 32]
    Fn.GATE_SMALL_DEFAULT.update(fuse=True, gate=True)          # "fused" at d = 32 means the kernels, whatever the default says
    store = synth.make_store(544, seed=2018)
    i1, i2, _ = synth.make_pairs(544, seed=777, limit=B)
    pb = packed.pack_from_store(packed.MolStore(store), [i1, i2], device=dev)
    N = pb.n_rows
    res = dict(rows=N, pairs=B)
    if any(d != 32 for d in widths):
        res["layers"] = 4                                       # the depth of the d = 128 / 64 legs; d = 32 carries its own
    for d in widths:
        layers = 8 if d == 32 else 4
        fwd_entry, bwd_entry = (L.bmp_ggnn_gate_step_small_fwd, L.bmp_ggnn_gate_step_small_bwd) if d == 32 else \
            (L.bmp_ggnn_gate_step_tile_fwd, L.bmp_ggnn_gate_step_tile_bwd)
        f = lambda *s: (torch.randn(*s, device=dev) * 0.1)
        x = f(N, d).requires_grad_()
        dout = f(N, d)
        keep = (torch.rand(N, d, device=dev) >= 0.05).float() / 0.95
        r = {}
        for kind, kname in ((0, "fuse"), (1, "gate")):
            nu = (3 if kind == 0 else 1) * d
            W = [[f(4 * d, d).requires_grad_(), f(4, d).requires_grad_(), f(2 * d, nu).requires_grad_(), f(nu).requires_grad_()]
                 for _ in range(layers)]

            def step(l, fused, k):
                w = W[l]
                out = Fn.gate_step(x, w[0], w[1], w[2], w[3], kind, k, pb, fused)
                torch.autograd.grad(out, [x] + w, dout)

            for k, tag in ((None, ""), (keep, "_keep")) if kind == 0 else ((None, ""),):
                # the steps in turn (each with its own weights), the fused and the composed form alternating, reported per step
                tf, tc = timed_pair(lambda: [step(l, True, k) for l in range(layers)], lambda: [step(l, False, k) for l in range(layers)])
                r[f"{kname}_fused{tag}_fwd_bwd_per_step"] = {a: b / layers for a, b in tf.items()}
                r[f"{kname}_composed{tag}_fwd_bwd_per_step"] = {a: b / layers for a, b in tc.items()}
            # the bare fused launches
            w = [t.detach() for t in W[0]]
            WTp, AUp, Wnp, Unp = Fn.pack_k4(w[0]), Fn.pack_k4(w[2]), Fn.pack_k4(w[0].t()), Fn.pack_k4(w[2].t())
            e = lambda n: torch.empty(N, n, device=dev)
            m, act, hout, dh, gda = e(d), e(nu), e(d), e(d), e(4 * d + nu)
            xd = x.detach()
            r[f"{kname}_step_tile_fwd"] = timed(lambda: check(fwd_entry(
                kind, ptr(xd), pb.n_tiles, d, ptr(pb.csr_ptr), ptr(pb.csr_col), ptr(pb.csr_val), ptr(WTp), ptr(w[1]), ptr(AUp), ptr(w[3]),
                None, ptr(m), ptr(act), ptr(hout), stream()), "fwd"))
            r[f"{kname}_step_tile_bwd"] = timed(lambda: check(bwd_entry(
                kind, ptr(dout), ptr(xd), ptr(m), ptr(act), None, pb.n_tiles, d, ptr(pb.csrT_ptr), ptr(pb.csrT_col), ptr(pb.csrT_val),
                ptr(Wnp), ptr(Unp), ptr(dh), ptr(gda), stream()), "bwd"))
            r[f"{kname}_linear_wgrad_both"] = timed(lambda: (Fn._linear_wgrad(xd, gda), Fn._linear_wgrad(m, gda[:, 4 * d:], bias=False)))
        if d == 32:
            r["layers"] = layers
        res[f"d{d}"] = r
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
