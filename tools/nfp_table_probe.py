"""Times the NFP layer and the NFP readout at d = 64 and 128 on TILE-TABLE batches: forward plus backward (weight gradients
included) as the table kernels (csrc/bmp_nfp_table.hip) and as the row-wise entries (bmp_nfp_layer_fwd / _bwd, bmp_nfp_readout_fwd
/ _bwd with the listed weight gradient: what a table batch ran before the table kernels existed, picked by switching
``Fn.NFP_TABLE_DEFAULT`` off), in the same process on the same batch object: 1024 pairs of the DDI-shaped synthetic store in
(a) the encoder layout and (b) the encoder layout with de-duplication, 4 layers' worth of distinct weights, the readout at
o = d.  Four runs of 100 alternating calls after 10, medians with min and p90, by torch.cuda.Event.

The adoption rule is the project's (README, ggnn_dev paragraph): a width goes to the table kernels by default
(Fn.NFP_TABLE_DEFAULT) if the gain of the median exceeds the two forms' p90 - median spreads together in at least three of the
four runs, in both layouts, for the layer AND for the readout.

Report only: ms per replay of GraphedTrainStep at 32 pairs for a four-layer NFP + MLP model with the table kernels and with the
switch off; ms per 1024-pair training step (forward, loss, backward) of that model per instance, in the encoder layout and with
dedup, the table layouts with the switch on and off.

The driver opens no GPU itself: every leg -- the layer timing of one width, the readout timing of one width, a replay timing, the
step timing -- is a child process under a time limit of its own (tools/table_probe_lib.py), and the first leg that fails or runs
out of time ends the probe.  One JSON line per run, then one summary line.
python tools/nfp_table_probe.py [--runs 4] [--out FILE]          (profiles/nfp_table_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.join(ROOT, "tools")]
import table_probe_lib as T                                    # noqa: E402

WIDTHS, LAYERS, STEP_D = (64, 128), 4, 128
# (a layer or readout leg of one width makes 2 alternating timings per run, 8 in four runs)
LEG_SECONDS = {"layers": 8 * T.PAIR_SECONDS, "readout": 8 * T.PAIR_SECONDS, "replay": T.REPLAY_SECONDS, "step": 240}


class ReadoutPaths:
    """Fn.NFP_PATHS' readout counters under the names table_probe_lib counts by."""
    KEYS = {"fused": "readout_tile", "composed": "readout_rows"}

    def __init__(self, Fn):
        self.Fn = Fn

    def keys(self):
        return self.KEYS.keys()

    def __getitem__(self, k):
        return self.Fn.NFP_PATHS[self.KEYS[k]]


def _rand(dev):
    import torch
    return lambda *s: (torch.randn(*s, device=dev) * 0.1)


def layer_run(Fn, pb, nd, dev, d):
    import torch
    f = _rand(dev)
    x, dout = f(pb.n_rows, d).requires_grad_(), f(pb.n_rows, d)
    W = [[f(7, d, d).requires_grad_(), f(d).requires_grad_()] for _ in range(LAYERS)]

    def layer(l, table):
        Fn.NFP_TABLE_DEFAULT[d] = table
        out = Fn.NFPLayerFn.apply(x, *W[l], pb, nd, True)
        torch.autograd.grad(out, [x] + W[l], dout)

    return T.table_against_composed(Fn.NFP_LAYER_PATHS, layer, LAYERS)


def readout_run(Fn, pb, dev, d):
    import torch
    f = _rand(dev)
    x, dg = f(pb.n_rows, d).requires_grad_(), f(pb.n_mols, d)
    W = [[f(d, d).requires_grad_(), f(d).requires_grad_()] for _ in range(LAYERS)]

    def readout(l, table):
        Fn.NFP_TABLE_DEFAULT[d] = table
        g = Fn.NFPReadoutFn.apply(x, *W[l], pb, None, True)
        torch.autograd.grad(g, [x] + W[l], dg)

    return T.table_against_composed(ReadoutPaths(Fn), readout, LAYERS)


def leg_timing(what, d, runs):
    """One JSON line per run: the layer or the readout at width ``d`` in both table layouts."""
    from bmp import functional as Fn
    from bmp.nfp import nfp_derived
    dev, ds, i1, i2, _lab = T.world()
    batches = T.table_batches(ds, i1, i2)
    for run in range(runs):
        res = dict(run=run, what=what, d=d, pairs=T.B, layers=LAYERS)
        for name, eb in batches.items():
            pb = eb.pb_enc
            assert Fn.nfp_table_ok(pb, d) and Fn.nfp_table_ok(pb, d, d)
            r = layer_run(Fn, pb, nfp_derived(pb, enc=True), dev, d) if what == "layers" else readout_run(Fn, pb, dev, d)
            res[name] = dict(rows=pb.n_rows, tiles=pb.n_mtiles, **r)
        print(json.dumps(res), flush=True)


def _model(d, dev):
    import torch
    from bmp.predictor import build_pair_predictor
    torch.manual_seed(1)
    return build_pair_predictor(encoder="nfp", hidden_dim=d, out_dim=d, n_layers=LAYERS, attn=None).to(dev)


def leg_replay(d):
    """One JSON line: ms per replay of the recorded NFP + MLP training step at 32 pairs (load + replay, 200 of them after 20),
    with the switch off and on."""
    from bmp import functional as Fn
    dev, ds, i1, i2, lab = T.world()
    res = dict(replay32_nfp=True, d=d, layers=LAYERS)
    for table in (False, True):
        Fn.NFP_TABLE_DEFAULT.update({k: table for k in Fn.NFP_TABLE_DEFAULT})
        res["table" if table else "rows"] = T.replay_ms(Fn.NFP_LAYER_PATHS, ds, i1, i2, lab, _model(d, dev), table)
    print(json.dumps(res), flush=True)


def leg_step(d, layouts=("instance", "encoder", "encoder_dedup")):
    """One JSON line: ms per 1024-pair training step (forward, loss, backward; 30 after 5) of the NFP + MLP model per layout; the
    table layouts with the switch on and off.  (The per-instance batch is whole tiles: the switch does not reach it.)"""
    import numpy as np
    import torch
    from bmp import functional as Fn
    from bmp import packed
    dev, ds, i1, i2, lab = T.world()
    model = _model(d, dev)

    def timed(batch, t):
        ts = []
        for k in range(35):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            model.zero_grad()
            a.record(); model.forward_loss(batch, t=t).backward(); b.record(); b.synchronize()
            if k >= 5:
                ts.append(a.elapsed_time(b))
        return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), p90_ms=float(np.percentile(ts, 90)))

    res = dict(step1024_nfp=True, d=d, layers=LAYERS, pairs=T.B)
    if "instance" in layouts:
        res["instance"] = timed(*packed.pack_from_store_device(ds, [i1, i2], labels=lab))
    if len(layouts) > 1:
        from bmp import enclayout
        for name, dedup in (("encoder", False), ("encoder_dedup", True)):
            eb, t = enclayout.encode_from_store_device(ds, [i1, i2], labels=lab, dedup=dedup)
            for table in (False, True):
                Fn.NFP_TABLE_DEFAULT.update({k: table for k in Fn.NFP_TABLE_DEFAULT})
                res[f"{name}_{'table' if table else 'rows'}"] = dict(rows=eb.pb_enc.n_rows, **timed(eb, t))
    print(json.dumps(res), flush=True)


def main():
    runs = int(T.arg("--runs", 4))
    leg, d = T.arg("--leg"), int(T.arg("--d", 0))
    if leg in ("layers", "readout"):
        return leg_timing(leg, d, runs)
    if leg == "replay":
        return leg_replay(d)
    if leg == "step":
        return leg_step(d)
    if leg == "step_instance":                                  # (what a build of another commit can run too)
        return leg_step(d, ("instance",))
    legs = [(what, w, LEG_SECONDS[what]) for what in ("layers", "readout") for w in WIDTHS]
    legs += [("replay", w, LEG_SECONDS["replay"]) for w in WIDTHS] + [("step", STEP_D, LEG_SECONDS["step"])]
    lines = T.run_legs(__file__, legs, runs)
    if lines is None:
        return 1
    need = 3 if runs >= 4 else runs
    layouts = ("encoder", "encoder_dedup")
    timed = [l for l in lines if "run" in l]
    passes = {str(d): {f"{what}/{name}": sum(l[name]["passes"] for l in timed if l["d"] == d and l["what"] == what)
                       for what in ("layers", "readout") for name in layouts} for d in WIDTHS}
    adopt = {k: bool(min(v.values()) >= need) for k, v in passes.items()}
    T.finish(lines, dict(summary=True, runs=runs, passes=passes, adopt=adopt))
    return 0


if __name__ == "__main__":
    sys.exit(main())
