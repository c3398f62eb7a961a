"""Times the NFP layer launches (bmp_nfp_layer_tile_fwd / _tile_bwd, bmp_nfp_layer_wgrad, the readout per tile, and the row-wise forms) at d = 128 on a 1024-pair batch of
the DDI-shaped synthetic store and, in the same process and on the same batch, the fused RelGCN layer launches
(bmp_relgcn_layer_fwd / _bwd / _wgrad).  Medians over repeated launches after a warm-up, with the spread; also the count of
(32-row block, degree class) pairs per 64-row half tile, which a class-walking tile kernel's cost would rest on.
Prints one JSON line.  python tools/nfp_probe.py [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd")]
from bmp import functional as Fn, packed, synth, _lib          # noqa: E402
from bmp._lib import check, ptr, stream                        # noqa: E402
from bmp.nfp import nfp_derived                                # noqa: E402


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
    d, B = 128, 1024
    store = synth.make_store(544, seed=2018)
    i1, i2, _ = synth.make_pairs(544, seed=777, limit=B)
    pb = packed.pack_from_store(packed.MolStore(store), [i1, i2], device=dev)
    nd = nfp_derived(pb)
    N = pb.n_rows
    f = lambda *s: torch.randn(*s, device=dev) * 0.1
    x, dout = f(N, d), f(N, d)
    # ---- NFP
    WT, B_, Wnat = f(7, d, d), f(d), f(7, d, d)
    fv, out, dpre, dfv, dh = (torch.empty(N, d, device=dev) for _ in range(5))
    dWT, dB = torch.empty(7, d, d, device=dev), torch.empty(d, device=dev)
    nws = L.bmp_nfp_layer_wgrad_ws_floats(N, d, d)
    ws = torch.empty(nws, device=dev)
    res = {}
    res["nfp_layer_fwd"] = timed(lambda: check(L.bmp_nfp_layer_fwd(
        ptr(x), pb.n_tiles, d, d, ptr(pb.csr_ptr), ptr(pb.csr_col), ptr(pb.csr_val), ptr(nd["self_w"]), ptr(nd["deg_class"]),
        ptr(WT), ptr(B_), ptr(fv), ptr(out), stream()), "fwd"))
    res["nfp_layer_bwd"] = timed(lambda: check(L.bmp_nfp_layer_bwd(
        ptr(dout), ptr(out), pb.n_tiles, d, d, ptr(pb.csrT_ptr), ptr(pb.csrT_col), ptr(pb.csrT_val), ptr(nd["self_w"]),
        ptr(nd["deg_class"]), ptr(pb.row_w), ptr(Wnat), ptr(dpre), ptr(dfv), ptr(dh), stream()), "bwd"))
    for listed in (1, 0):
        res["nfp_layer_wgrad_listed" if listed else "nfp_layer_wgrad_rowwise"] = timed(lambda: check(L.bmp_nfp_layer_wgrad(
            ptr(fv), ptr(dpre), N, d, d, ptr(nd["deg_rows"]), ptr(nd["deg_cnt"]), ptr(dWT), ptr(dB), listed, ptr(ws), nws, stream()), "wgrad"))
    WTp = torch.stack([Fn.pack_k4(WT[k]) for k in range(7)]); Wnp = torch.stack([Fn.pack_k4(Wnat[k]) for k in range(7)])
    res["nfp_layer_tile_fwd"] = timed(lambda: check(L.bmp_nfp_layer_tile_fwd(
        ptr(x), pb.n_tiles, d, ptr(pb.csr_ptr), ptr(pb.csr_col), ptr(pb.csr_val), ptr(nd["self_w"]), ptr(nd["deg_class"]),
        ptr(WTp), ptr(B_), ptr(fv), ptr(out), stream()), "tile fwd"))
    res["nfp_layer_tile_bwd"] = timed(lambda: check(L.bmp_nfp_layer_tile_bwd(
        ptr(dout), ptr(out), pb.n_tiles, d, ptr(pb.csrT_ptr), ptr(pb.csrT_col), ptr(pb.csrT_val), ptr(nd["self_w"]),
        ptr(nd["deg_class"]), ptr(pb.row_w), ptr(Wnp), ptr(dpre), ptr(dh), stream()), "tile bwd"))
    WoTp, Wonp, bo = Fn.pack_k4(f(d, d)), Fn.pack_k4(f(d, d)), f(d)
    sbuf, g, dg = torch.empty(N, d, device=dev), torch.empty(pb.n_mols, d, device=dev), f(pb.n_mols, d)
    res["nfp_readout_tile_fwd"] = timed(lambda: check(L.bmp_nfp_readout_tile_fwd(
        ptr(out), pb.n_tiles, d, d, ptr(WoTp), ptr(bo), ptr(pb.row_w), ptr(pb.row_mol), ptr(sbuf), ptr(g), 0, stream()), "ro fwd"))
    nwr = L.bmp_nfp_readout_bwd_ws_floats(N, d, d)
    wsr, dWo, dbo = torch.empty(nwr, device=dev), torch.empty(d, d, device=dev), torch.empty(d, device=dev)
    res["nfp_readout_tile_bwd_with_wgrad"] = timed(lambda: check(L.bmp_nfp_readout_tile_bwd(
        ptr(dg), ptr(out), ptr(sbuf), pb.n_tiles, d, d, ptr(Wonp), ptr(pb.row_w), ptr(pb.row_mol), ptr(dh), ptr(dWo), ptr(dbo),
        ptr(wsr), nwr, stream()), "ro bwd"))
    # ---- RelGCN layer (the unchanged library code), same batch
    WTp, WsTp = Fn.pack_k4(f(4 * d, d)), Fn.pack_k4(f(d, d))
    Wnat_p, Ws_p = Fn.pack_k4(f(d, 4 * d)), Fn.pack_k4(f(d, d))
    bE, bs = f(4, d), f(d)
    o, wdeg = Fn._rel_fwd(x, pb, WTp, bE, WsTp, bs, 2)
    res["relgcn_layer_fwd"] = timed(lambda: Fn._rel_fwd(x, pb, WTp, bE, WsTp, bs, 2, bufs=(o, wdeg)))
    gda, dx = torch.empty(N, 5 * d, device=dev), torch.empty(N, d, device=dev)
    tri, trc, skip = Fn.step_lists(pb, N, d)
    mt = Fn._rel_mt(pb)
    res["relgcn_layer_bwd"] = timed(lambda: check(L.bmp_relgcn_layer_bwd(
        ptr(dout), ptr(o), 2, pb.n_mtiles, d, ptr(pb.csrT_ptr), ptr(pb.csrT_col), ptr(pb.csrT_val), ptr(Wnat_p), ptr(Ws_p), ptr(dx),
        ptr(gda), ptr(mt[0]), ptr(mt[1]), pb.n_rows, skip, stream()), "rel bwd"))
    o1, dbE, cs = torch.empty(d, 5 * d, device=dev), torch.empty(4, d, device=dev), torch.empty(5 * d, device=dev)
    nw2 = L.bmp_relgcn_layer_wgrad_ws_floats(N, d)
    ws2 = torch.empty(nw2, device=dev)
    res["relgcn_layer_wgrad"] = timed(lambda: check(L.bmp_relgcn_layer_wgrad(
        ptr(x), ptr(wdeg), ptr(gda), N, d, ptr(o1), ptr(dbE), ptr(cs), 0, ptr(tri), ptr(trc), ptr(ws2), nw2, stream()), "rel wgrad"))
    # ---- (block, class) pairs per 64-row half tile, rows in packed order and sorted by class
    cls = nd["deg_class"].cpu().numpy().reshape(-1, 64)
    live = (pb.row_w.cpu().numpy().reshape(-1, 64) > 0).any(axis=1) | (cls > 0).any(axis=1)
    unsorted = [sum(len(set(h[b:b + 32][h[b:b + 32] > 0])) for b in (0, 32)) for h in cls[live]]
    srt = [sum(len(set(s[b:b + 32][s[b:b + 32] > 0])) for b in (0, 32)) for s in (np.sort(h)[::-1] for h in cls[live])]
    res["block_class_pairs_per_half"] = dict(packed_order_mean=float(np.mean(unsorted)), sorted_mean=float(np.mean(srt)),
                                             sorted_max=int(np.max(srt)), halves=int(live.sum()))
    res["class_share"] = [float((cls == k).mean()) for k in range(8)]
    res["rows"], res["d"], res["pairs"] = N, d, B
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
