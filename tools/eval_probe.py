"""What an epoch's evaluation costs at the reference's default batch of 32 pairs, and what the recorded + on-device evaluation
(bmp.dp.GraphedPredict, bmp.trainer.ScoreSink) takes off it.

Legs (each a child process under a time limit of its own; the driver opens no GPU and starts nothing behind a leg that failed):

  evaluate MODEL 32 static     ms per batch inside ``evaluate`` over a 4096-pair set, three forms called in turn: "recorded"
                               (graphed + on device), "eager_sink" (launch by launch + on device) and "parent": a checkout of
                               the PARENT commit (``--parent DIR``, its library built) running its own ``evaluate`` on its own
                               copy of the same batches -- never this tree with its switches off.  The parent's package is
                               loaded beside this one under the name ``bmp_parent``; all three forms must return the same dict.
  epoch MODEL                  wall-clock of one ``fit`` epoch (4096 training pairs, eval_train=True, 1024 validation pairs),
                               split into training and evaluation, this tree with both switches on against the parent.
  evaluate c2 1024 instance    report only: the GPU-bound batch, where the sink removes two host round trips per batch and is
                               expected to gain little; it must not lose.

Adoption rule (the project's): medians of ``--runs`` (4) runs of ``--calls`` (100) alternating calls; a form passes a run when its
gain over the parent exceeds the two forms' p90 - median spreads together; it is adopted when it passes in at least three of the
four runs.  ``--out FILE`` keeps every line (profiles/eval_probe.json).

  python tools/eval_probe.py --parent /path/to/parent/checkout [--models ref_ntn,c2] [--legs evaluate,epoch,big] [--out FILE]
      [--with-host-form 1]     also times this tree's own launch-by-launch path through the host (a diagnostic: two packages in
                               one process hold two sets of side streams, which the runtime maps onto a handful of queues)
"""
import importlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gcn-bmp_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
from table_probe_lib import arg, finish          # noqa: E402

CFG = {"ref_ntn": dict(hidden_dim=32, out_dim=16, n_layers=8, attn="nie", weight_tying=False, sim_method="ntn", mlp_hidden=()),
       "c2": dict(hidden_dim=128, out_dim=128, n_layers=4, attn="nie")}
N_SET, N_VALID = 4096, 1024
LEG_SECONDS = dict(evaluate=420, epoch=240, big=240)


def parent_package(path):
    """The parent checkout's ``bmp`` package under the name ``bmp_parent`` (its relative imports stay inside it, and its
    ``_lib`` loads the library built beside it)."""
    pkg = os.path.join(path, "gcn-bmp_amd", "bmp")
    spec = importlib.util.spec_from_file_location("bmp_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["bmp_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def setup(pkg, name, batch, layout):
    """Store, pairs, model and optimizer built by the package ``pkg`` (same seeds: the two packages hold the same numbers)."""
    import torch
    synth, packed, trainer, dp, predictor = (importlib.import_module(f"{pkg}.{m}") for m in ("synth", "packed", "trainer", "dp", "predictor"))
    dev = torch.device("cuda:0")
    ds = packed.DeviceMolStore(packed.MolStore(synth.make_store(544, seed=2018)), dev)
    i1, i2, lab = synth.make_pairs(544, seed=777, limit=N_SET + N_VALID)
    lab = lab.reshape(-1, 1)
    torch.manual_seed(1)
    model = predictor.build_pair_predictor(**CFG[name]).to(dev)
    opt = dp.FlatAdam(model, alpha=1e-3)
    make = lambda lo, hi: trainer.PairBatches(ds, i1[lo:hi], i2[lo:hi], lab[lo:hi], batch_size=batch, layout=layout)
    return SimpleNamespace(trainer=trainer, dp=dp, model=model, opt=opt, make=make, file=trainer.__file__)


def emit(line):
    """A leg's result line: to the output as it arrives, and to the file the driver reads when the leg has ended."""
    print(json.dumps(line), flush=True)
    if arg("--lines"):
        with open(arg("--lines"), "a") as fh:
            fh.write(json.dumps(line) + "\n")


def stats(ts):
    import numpy as np
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), p90_ms=float(np.percentile(ts, 90)))


def rule(form, base):
    gain = base["median_ms"] - form["median_ms"]
    spread = (form["p90_ms"] - form["median_ms"]) + (base["p90_ms"] - base["median_ms"])
    return dict(gain_ms=gain, spreads_ms=spread, passes=bool(gain > spread), loses=bool(-gain > spread))


def leg_evaluate(name, batch, layout, runs, calls):
    import torch
    here, base = setup("bmp", name, batch, layout), setup("bmp_parent", name, batch, layout)
    assert os.path.realpath(here.file) != os.path.realpath(base.file), "--parent is this tree"
    sets = {k: w.make(0, N_SET) for k, w in (("here", here), ("parent", base))}
    nb = len(sets["here"])
    ev = lambda w, s, **kw: w.trainer.evaluate(w.model, s, lossfun=w.model.loss, opt=w.opt, **kw)
    forms = {}
    if layout == "static":
        gp = here.dp.GraphedPredict(here.model, here.opt)
        forms["recorded"] = lambda: ev(here, sets["here"], graphed=gp)
    forms["eager_sink"] = lambda: ev(here, sets["here"], graphed=False, on_device=True)
    if arg("--with-host-form"):      # diagnostic, never the baseline: this tree's own path through the host, in this process
        forms["this_tree_host"] = lambda: ev(here, sets["here"], graphed=False, on_device=False)
    forms["parent"] = lambda: ev(base, sets["parent"])
    res = {k: f() for k, f in forms.items()}
    for _ in range(2):
        res = {k: f() for k, f in forms.items()}
    assert all(r == res["parent"] for r in res.values()), res          # the three forms computed the same thing
    lines = []
    for run in range(runs):
        ts = {k: [] for k in forms}
        for _ in range(calls):
            for k, f in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3 / nb)
        st = {k: stats(v) for k, v in ts.items()}
        line = dict(leg="evaluate", model=name, batch=batch, layout=layout, run=run, calls=calls, batches_per_call=nb,
                    what="ms per batch inside evaluate", **st)
        for k in forms:
            if k != "parent":
                line[k + "_vs_parent"] = rule(st[k], st["parent"])
        lines.append(line)
        emit(line)
    summary = dict(leg="evaluate_summary", model=name, batch=batch, layout=layout, runs=runs, calls=calls)
    for k in forms:
        if k != "parent":
            n_pass = sum(l[k + "_vs_parent"]["passes"] for l in lines)
            n_lose = sum(l[k + "_vs_parent"]["loses"] for l in lines)
            summary[k] = dict(passes_runs=n_pass, loses_runs=n_lose, adopted=bool(runs >= 4 and n_pass >= 3),
                              median_ms=sorted(l[k]["median_ms"] for l in lines)[len(lines) // 2])
    summary["parent"] = dict(median_ms=sorted(l["parent"]["median_ms"] for l in lines)[len(lines) // 2])
    emit(summary)


def leg_epoch(name, epochs):
    """fit for ``epochs`` epochs (the first one records the graphs and is left out): seconds per epoch, in evaluate and outside."""
    import numpy as np
    import torch
    out = {}
    for who, pkg in (("recorded_on_device", "bmp"), ("parent", "bmp_parent")):
        w = setup(pkg, name, 32, "static")
        if who != "parent":
            w.trainer.EVAL_GRAPH_DEFAULT = w.trainer.EVAL_ON_DEVICE_DEFAULT = True
        inner, spent, marks = w.trainer.evaluate, [0.0], []

        def timed(*a, _inner=inner, _spent=spent, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = _inner(*a, **kw)
            _spent[0] += time.perf_counter() - t0
            return r

        def report(log, _spent=spent, _marks=marks):
            torch.cuda.synchronize()
            _marks.append((time.perf_counter(), _spent[0]))

        w.trainer.evaluate = timed
        torch.cuda.synchronize()
        marks.append((time.perf_counter(), 0.0))
        logs = w.trainer.fit(w.model, w.opt, w.make(0, N_SET), w.make(N_SET, N_SET + N_VALID), epochs=epochs, eval_train=True,
                             report=report)
        w.trainer.evaluate = inner
        tot = [b[0] - a[0] for a, b in zip(marks[1:-1], marks[2:])]
        evs = [b[1] - a[1] for a, b in zip(marks[1:-1], marks[2:])]
        out[who] = dict(epoch_s=float(np.median(tot)), evaluate_s=float(np.median(evs)),
                        training_s=float(np.median([t - e for t, e in zip(tot, evs)])), first_epoch_s=marks[1][0] - marks[0][0],
                        val_loss=[l["validation/main/loss"] for l in logs])
    same = out["parent"]["val_loss"] == out["recorded_on_device"]["val_loss"]
    emit(dict(leg="epoch", model=name, train_pairs=N_SET, valid_pairs=N_VALID, batch=32, epochs_timed=epochs - 1,
              same_validation_losses=same, **out))


def child():
    parent_package(arg("--parent"))
    leg, name = arg("--leg"), arg("--model")
    runs, calls = int(arg("--runs", 4)), int(arg("--calls", 100))
    if leg == "evaluate":
        leg_evaluate(name, 32, "static", runs, calls)
    elif leg == "big":
        leg_evaluate(name, 1024, "instance", runs, calls)
    else:
        leg_epoch(name, int(arg("--epochs", 4)))


def main():
    if arg("--leg"):
        return child()
    if not arg("--parent") or not os.path.exists(os.path.join(arg("--parent"), "gcn-bmp_amd", "bmp", "libbmp_hip.so")):
        sys.exit("--parent DIR: a checkout of the parent commit with its library built (the baseline is never this tree)")
    models = arg("--models", "ref_ntn,c2").split(",")
    legs = arg("--legs", "evaluate,epoch,big").split(",")
    todo = [(l, m) for l in ("evaluate", "epoch") if l in legs for m in models] + ([("big", "c2")] if "big" in legs else [])
    lines = []
    for leg, model in todo:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--model", model, "--parent", arg("--parent"),
               "--runs", arg("--runs", "4"), "--calls", arg("--calls", "100"), "--epochs", arg("--epochs", "4")]
        cmd += ["--with-host-form", "1"] if arg("--with-host-form") else []
        seconds = int(arg("--seconds", LEG_SECONDS[leg]))
        with tempfile.NamedTemporaryFile(suffix=".jsonl") as tmp:        # (the leg prints its lines itself, as they arrive)
            try:
                rc = subprocess.run(cmd + ["--lines", tmp.name], timeout=seconds).returncode
            except subprocess.TimeoutExpired:
                rc = f"no end within {seconds} s"
            lines += [json.loads(l) for l in open(tmp.name) if l.startswith("{")]
        if rc != 0:
            lines.append(dict(error=f"leg {leg} {model}: {rc if isinstance(rc, str) else 'exit status %d' % rc}"))
            print(json.dumps(lines[-1]), flush=True)
            break
    failed = any("error" in l for l in lines)
    finish(lines, dict(leg="done", legs=[f"{l}:{m}" for l, m in todo], failed=failed))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
