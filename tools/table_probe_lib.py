"""What the tile-table probes share (tools/gate_table_probe.py, loop_table_probe.py, jk_table_probe.py, gin_table_probe.py): the
1024-pair world, the alternating timing of two forms of the same work (also tools/gate_probe.py's and tools/jk_probe.py's), the
per-layer gain / spread / passes arithmetic of the adoption rule, the replay timing of a recorded training step and the driver
that runs every leg of a probe as a child process under a time limit of its own.  Importing this module opens no GPU."""
import json
import os
import subprocess
import sys
import time

B = 1024
# What a leg's time limit is sized from: tools/jk_table_probe.py and tools/gin_table_probe.py gave the timing of one width 240 s
# for the 8 alternating timings of its four runs, 30 s each, and a replay timing (2 x 220 recorded steps) 180 s.
PAIR_SECONDS, REPLAY_SECONDS = 30, 180


def world():
    """(device, device store, i1, i2, labels) of 1024 pairs of the DDI-shaped synthetic store."""
    import torch
    from bmp import packed, synth
    dev = torch.device("cuda:0")
    store = synth.make_store(544, seed=2018)
    i1, i2, lab = synth.make_pairs(544, seed=777, limit=B)
    return dev, packed.DeviceMolStore(packed.MolStore(store), dev), i1, i2, lab.reshape(-1, 1)


def table_batches(ds, i1, i2):
    """The pairs in the two table layouts: the encoder layout, and the encoder layout with de-duplication."""
    from bmp import enclayout
    return {"encoder": enclayout.encode_from_store_device(ds, [i1, i2]),
            "encoder_dedup": enclayout.encode_from_store_device(ds, [i1, i2], dedup=True)}


def stats(ts):
    import numpy as np
    ts = np.array(ts)
    return dict(median_us=float(np.median(ts)), min_us=float(ts.min()), p90_us=float(np.percentile(ts, 90)))


def timed_pair(fa, fb, warm=10, reps=100):
    """Times two forms of the same work by torch.cuda.Event, alternating them call by call: what else runs on the host and the
    card's clock state meet both alike, and 100 calls of each make a window of seconds, not milliseconds."""
    import torch
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
    return stats(ta), stats(tb)


def table_against_composed(paths, step, layers):
    """``step(l, fused)`` runs layer l forward and backward, counted in the family's ``paths``.  Per layer: the two forms'
    timings, the gain of the median and the two p90 - median spreads together; the run passes when the gain exceeds the spreads."""
    before = dict(paths)
    tf, tc = timed_pair(lambda: [step(l, True) for l in range(layers)], lambda: [step(l, False) for l in range(layers)])
    tk = {a: paths[a] - before[a] for a in before}
    assert tk["fused"] == tk["composed"] == 110 * layers, tk          # the two forms really ran
    tf, tc = ({a: b / layers for a, b in t.items()} for t in (tf, tc))
    gain = tc["median_us"] - tf["median_us"]
    spread = (tf["p90_us"] - tf["median_us"]) + (tc["p90_us"] - tc["median_us"])
    return dict(table=tf, composed=tc, gain_us=gain, spreads_us=spread, passes=bool(gain > spread))


def replay_ms(paths, ds, i1, i2, lab, model, table):
    """ms per replay of the model's recorded training step at 32 pairs (load + replay, 200 of them after 20); ``table`` says
    which form the switch, set by the caller, must have recorded."""
    import numpy as np
    import torch
    from bmp import packed
    from bmp.dp import FlatAdam, GraphedTrainStep
    opt = FlatAdam(model, alpha=1e-3)
    sb = packed.StaticPairBatch(ds, 32)
    stepper = GraphedTrainStep(model, opt)
    before = dict(paths)
    ts = []
    for k in range(220):
        sl = slice(32 * (k % 32), 32 * (k % 32) + 32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sb.load([i1[sl], i2[sl]], lab[sl]); stepper(sb); torch.cuda.synchronize()
        if k >= 20:
            ts.append((time.perf_counter() - t0) * 1e3)
    tk = {a: paths[a] - before[a] for a in before}
    assert (tk["composed"] == 0) == table and (tk["fused"] == 0) != table, (table, tk)      # what was recorded
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), p90_ms=float(np.percentile(ts, 90)))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def run_legs(script, legs, runs, quiet=()):
    """The driver, which opens no GPU itself: each (leg, d, seconds) runs ``script --leg LEG --d D --runs RUNS`` as a process of
    its own under its time limit and its JSON lines are printed as they arrive, but those of the ``quiet`` legs, which the caller
    folds into its summary line.  All lines, or None behind the first leg that failed or ran out of time: nothing more is
    started on the card then."""
    lines = []
    for leg, d, seconds in legs:
        cmd = [sys.executable, os.path.abspath(script), "--leg", leg, "--d", str(d), "--runs", str(runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(error=f"leg {leg} d={d}: no end within {seconds} s")), flush=True)
            return None
        if r.returncode != 0:
            print(json.dumps(dict(error=f"leg {leg} d={d}: exit status {r.returncode}", tail=r.stderr[-1500:])), flush=True)
            return None
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                if leg not in quiet:
                    print(l, flush=True)
                lines.append(json.loads(l))
    return lines


def finish(lines, summary):
    """Prints the summary line behind the legs' lines and writes them all to ``--out``."""
    print(json.dumps(summary), flush=True)
    if arg("--out"):
        with open(arg("--out"), "w") as fh:
            for l in lines + [summary]:
                fh.write(json.dumps(l) + "\n")
