"""Times the layer-aggregator launches (bmp_layer_agg_fwd / bmp_layer_agg_bwd) alone, at the row count of a 1024-pair batch
of the DDI-shaped synthetic store: the C2 shape (d = 128, T = 4) and the shape of the reference's recorded run (d = 32,
T = 8), both modes, the attn backward with the softmax recomputed and with it kept in aux.  Medians over repeated launches
after a warm-up, with the spread; bytes the launch must move ((T+1) n d 4 forward, (2T+1) n d 4 backward with p recomputed,
plus aux where one is kept) and the GB/s that makes.  Prints one JSON line.  python tools/agg_probe.py [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd")]
from bmp import functional as Fn, packed, synth, _lib          # noqa: E402
from bmp._lib import check, ptr, stream                        # noqa: E402


def timed(fn, warm=5, reps=40):
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


def with_rate(t, nbytes):
    t["bytes"] = int(nbytes)
    t["GBps"] = nbytes / (t["median_us"] * 1e-6) / 1e9
    return t


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    store = synth.make_store(544, seed=2018)
    i1, i2, _ = synth.make_pairs(544, seed=777, limit=1024)
    N = packed.pack_from_store(packed.MolStore(store), [i1, i2], device=dev).n_rows
    res = {"rows": N}
    for d, T in ((128, 4), (32, 8)):
        f = lambda *s: torch.randn(*s, device=dev) * 0.5
        hs, dhs = [f(N, d) for _ in range(T)], [torch.empty(N, d, device=dev) for _ in range(T)]
        hp, dhp = Fn._ptr_array(hs), Fn._ptr_array(dhs)
        W, b, y, dy = f(T, T), f(T), torch.empty(N, d, device=dev), f(N, d)
        mask = torch.empty(N * d, dtype=torch.uint8, device=dev)
        pk = torch.empty(T, N, d, device=dev)
        dW, db = torch.empty(T, T, device=dev), torch.empty(T, device=dev)
        nws = L.bmp_layer_agg_ws_floats(N, d, T)
        ws = torch.empty(max(nws, 4), device=dev)
        e = N * d * 4
        r = {}
        r["max_fwd"] = with_rate(timed(lambda: check(L.bmp_layer_agg_fwd(
            hp, T, N, d, 0, None, None, ptr(y), ptr(mask), stream()), "max fwd")), (T + 1) * e + N * d)
        r["max_bwd"] = with_rate(timed(lambda: check(L.bmp_layer_agg_bwd(
            ptr(dy), None, T, N, d, 0, None, None, ptr(mask), dhp, None, None, 0, None, 0, stream()), "max bwd")), (T + 1) * e + N * d)
        r["attn_fwd"] = with_rate(timed(lambda: check(L.bmp_layer_agg_fwd(
            hp, T, N, d, 1, ptr(W), ptr(b), ptr(y), None, stream()), "attn fwd")), (T + 1) * e)
        r["attn_fwd_keep_p"] = with_rate(timed(lambda: check(L.bmp_layer_agg_fwd(
            hp, T, N, d, 1, ptr(W), ptr(b), ptr(y), ptr(pk), stream()), "attn fwd keep")), (2 * T + 1) * e)
        r["attn_bwd_recompute"] = with_rate(timed(lambda: check(L.bmp_layer_agg_bwd(
            ptr(dy), hp, T, N, d, 1, ptr(W), ptr(b), None, dhp, ptr(dW), ptr(db), 0, ptr(ws), nws, stream()), "attn bwd")),
            (2 * T + 1) * e)
        r["attn_bwd_kept_p"] = with_rate(timed(lambda: check(L.bmp_layer_agg_bwd(
            ptr(dy), hp, T, N, d, 1, ptr(W), ptr(b), ptr(pk), dhp, ptr(dW), ptr(db), 0, ptr(ws), nws, stream()), "attn bwd kept")),
            (3 * T + 1) * e)
        res[f"d{d}_T{T}"] = r
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
