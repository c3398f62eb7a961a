"""What the GPU tests of the tile-table families share (tests/test_gpu_ggate_enc.py, test_gpu_ggdev_enc.py, test_gpu_jk_table.py,
test_gpu_gin_table.py): the tables, the stride case, the two pair worlds and the fixed-shape world; the path counters and the
switch; and the bodies every family runs, as plain functions that take what varies between the families as arguments.  A family
file keeps its operands, its float64 restatement, its two C-ABI callers and its model factories, and binds them here.

Tolerances, all the project's: 1e-5 between two float32 forms of the same step, 1e-4 for parameters after several replayed steps
(test_gpu_static_batch.py), 1e-3 of the largest gradient as the floor of a parameter's scale (test_gpu_enclayout.py at full size).
Importing this module opens no GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

from enc_tables import COUNTS, TABLES, _hand_store
from parity_util import close
from test_gpu_ops import dev, to_dev                   # noqa: F401 (the family files take both from here or from there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


# ---- data ----
def table(name):
    """Host EncBatch without dedup of one of the three tables of tests/enc_tables.py, or of "dense" (one four-block tile whose
    CSR does not fit the staging in LDS), its properties asserted."""
    if name not in _CACHE:
        from bmp import enclayout, packed
        if name == "dense":
            import ggate32_ref as R
            ms, inst, n_cu = packed.MolStore(R._dense_store()), [0], 256
        else:
            ms = packed.MolStore(_hand_store())
            inst, n_cu = TABLES[name]
        eb = enclayout.encode_from_store(ms, [np.asarray(inst)], dedup=False, n_cu=n_cu)
        pl = enclayout.plan_enc_numpy(ms.n_atoms, ms.nedges, np.asarray(inst), False, n_cu)
        nb, r0 = pl["mt_nblk"].tolist(), pl["mt_row0"]
        n, row0, tile, pad = pl["n"], pl["row0"], pl["tile"], pl["enc_pad"]
        per_tile = np.bincount(tile, minlength=len(nb))
        off = row0 - r0[tile]
        if name == "own":
            assert nb == [4, 4, 3, 3, 2, 2, 2, 1, 1, 1, 1]
            at = lambda k: int(pad[list(n).index(k)] - r0[tile[list(n).index(k)]])
            assert at(31) == 31 and nb[tile[list(n).index(31)]] == 1          # the last row of a one-block tile
            assert at(32) == 32 and nb[tile[list(n).index(32)]] == 2          # the first row of a second block
            assert at(127) == 127 and nb[tile[list(n).index(127)]] == 4       # row 127 of a full tile
            assert per_tile.tolist()[-2:] == [0, 0] and (per_tile[:-2] >= 1).all()      # two molecule-free filler tiles
        elif name == "shared":
            assert sorted(per_tile[per_tile > 0].tolist()) == [1, 2, 2, 2, 3]       # tiles shared by two or three molecules
            u = list(n).index(32)
            assert off[u] == 95 and off[u] + n[u] > 96                        # starts at tile row 95, crosses the boundary at 96
        elif name == "seven":
            assert nb == [2, 1, 1] and per_tile.tolist() == [7, 0, 0]
        else:
            ecap = int(re.search(r"#define FZ_ECAP (\d+)", open(os.path.join(ROOT, "gcn-bmp_amd", "csrc", "bmp_tile.h")).read()).group(1))
            assert ecap == R.STAGED_CSR_ENTRIES and nb == [4] and eb.pb_enc.n_rows == 128
            assert int(eb.pb_enc.csr_ptr[128]) > ecap and int(eb.pb_enc.csrT_ptr[128]) > ecap
        assert eb.pb_enc.mt_row0 is not None and eb.pb_enc.tile_stride == 0 and not eb.pb_enc.oversized
        _CACHE[name] = eb
    return _CACHE[name]


def table_on_device(name):
    """The table's batch on the device; its tiles abut and hold every row once, under 800 rows."""
    pb = to_dev(table(name).pb_enc)
    cover = np.zeros(pb.n_rows, dtype=int)
    for a, k in zip(pb.mt_row0.cpu().numpy(), pb.mt_nblk.cpu().numpy()):
        cover[a:a + 32 * k] += 1
    assert (cover == 1).all() and pb.n_rows < 800
    return pb


def dense_adj(pb):
    """(1, 4, N, N) float64 adjacency of the batch's rows from its CSR: adj[0, e, dst, src] = val."""
    N = pb.n_rows
    ptr_, col, val = pb.csr_ptr.numpy(), pb.csr_col.numpy(), pb.csr_val.numpy()
    adj = np.zeros((1, 4, N, N))
    dst = np.repeat(np.arange(N), np.diff(ptr_[:N + 1]))
    adj[0, col & 3, dst, col >> 2] = val
    return adj


STRIDE_ROWS, CANARY_ROWS = 384, 128
STRIDE_BLOCKS = {(20, 40, 70): [1, 2, 3], (20, 70, 120): [1, 3, 4]}          # the live blocks of the three tiles


def stride_case(ns):
    """Three tiles at the fixed stride 128: molecules of ``ns`` atoms (chains, cycling bond types) and their pad rows.
    (csr, csrT, mt_row0, mt_nblk, live-row mask); N = 384."""
    N = STRIDE_ROWS
    dst, src, typ = [], [], []
    for t, n in enumerate(ns):
        for i in range(n - 1):
            a, b, e = 128 * t + i, 128 * t + i + 1, (i + t) % 4
            dst += [a, b]; src += [b, a]; typ += [e, e]
    dst, src, typ = np.array(dst), np.array(src), np.array(typ)

    def build(major, minor):
        order = np.lexsort((typ, minor, major))
        p_ = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(np.bincount(major, minlength=N), out=p_[1:])
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev())
        return i32(p_), i32((minor[order] << 2) | typ[order]), torch.ones(len(order), device=dev())

    nblk = [(n + 1 + 31) // 32 for n in ns]
    assert nblk == STRIDE_BLOCKS[tuple(ns)]
    live = np.zeros(N, dtype=bool)
    for t, k in enumerate(nblk):
        live[128 * t:128 * t + 32 * k] = True
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev())
    return build(dst, src), build(src, dst), i32([0, 128, 256]), i32(nblk), torch.from_numpy(live).to(dev())


def nan_dead(x, live):
    """``x`` with the dead rows NaN: rows no kernel may read."""
    return torch.where(live[:, None], x, torch.full_like(x, float("nan")))


def nan_rows(n):
    """A written array of the stride case prefilled with NaN, with a 128-row canary behind mt_rows."""
    return torch.full((STRIDE_ROWS + CANARY_ROWS, n), float("nan"), device=dev())


LAB = (np.arange(13).reshape(-1, 1) % 2).astype(np.int32)


def world(which):
    """One of the two 13-pair worlds, every molecule on both sides and several times: "synthetic", the 9-molecule
    heavy-repetition set of test_gpu_enclayout.py, or "hand", the hand-made store of tests/enc_tables.py."""
    if ("world", which) not in _CACHE:
        from bmp import packed, synth
        if which == "synthetic":
            store = synth.make_store(9, seed=31, n_lo=2, n_hi=60, n_mean=16)
            I1, I2 = [0, 1, 2, 0, 3, 3, 8, 1, 0, 5, 5, 2, 6], [1, 0, 0, 0, 4, 3, 1, 8, 7, 5, 2, 2, 6]
            counts = [m.n for m in store]
        else:
            store, counts = _hand_store(), COUNTS
            I1, I2 = [0, 1, 2, 8, 3, 3, 9, 1, 7, 5, 5, 4, 6], [1, 0, 8, 8, 4, 3, 1, 9, 0, 5, 2, 7, 6]
        ms = packed.MolStore(store)
        _CACHE[("world", which)] = types.SimpleNamespace(which=which, store=store, ms=ms, ds=packed.DeviceMolStore(ms, dev()),
                                                         I1=np.array(I1), I2=np.array(I2), counts=counts)
    return _CACHE[("world", which)]


def batches(w, dedup, n_cu):
    """(per-instance batch, its labels, encoder-layout batch, its labels) of the world's pairs."""
    from bmp import enclayout, packed
    pb, t = packed.pack_from_store_device(w.ds, [w.I1, w.I2], labels=LAB)
    eb, t2 = enclayout.encode_from_store_device(w.ds, [w.I1, w.I2], labels=LAB, dedup=dedup, n_cu=n_cu)
    assert eb.n_encoded == (len(w.store) if dedup else 26)
    nb = eb.pb_enc.mt_nblk.cpu().numpy()
    assert nb.min() >= 1 and eb.pb_enc.mt_row0 is not None and not eb.pb_enc.oversized
    if w.which == "synthetic":
        assert nb.max() <= 4 and (n_cu != 5 or nb.max() >= 2)
    else:
        assert nb.max() == 4
    return pb, t, eb, t2


def pair_run(model, batch, t, backward=True):
    from bmp.snapshot import grad_dict
    model.zero_grad()
    y = model(batch)
    if backward:
        model.loss(y, t).backward()
    return dict(y=y.detach(), g1=model.g1.detach(), g2=model.g2.detach(), grads=grad_dict(model) if backward else {})


def atoms_by_molecule(w, rows, pb):
    """The real atoms' rows of a row tensor on ``pb``, molecule by molecule in instance order."""
    r0 = pb.mol_row0.cpu().long().tolist()
    return torch.cat([rows[r0[i]:r0[i] + w.counts[k]] for i, k in enumerate(np.concatenate((w.I1, w.I2)))])


def static_world():
    """(device store, its molecules tallest first, their sizes): sixteen tall, sixteen short, sixteen between."""
    if "static" not in _CACHE:
        from bmp import packed, synth
        store = (synth.make_store(16, seed=3, n_lo=70, n_hi=120, n_mean=95) + synth.make_store(16, seed=4, n_lo=3, n_hi=28, n_mean=12)
                 + synth.make_store(16, seed=5, n_lo=20, n_hi=70, n_mean=40))
        ds = packed.DeviceMolStore(packed.MolStore(store), dev())
        by_size = np.argsort([-m.n for m in store], kind="stable")
        _CACHE["static"] = (ds, by_size, [m.n for m in store])
    return _CACHE["static"]


# ---- switches and counters ----
def took(paths, fn):
    """(fn(), what it added to the family's ``*_PATHS`` counters)."""
    before = dict(paths)
    out = fn()
    return out, {k: paths[k] - before[k] for k in before}


def force_on(monkeypatch, *defaults):
    """Every key of the family's ``*_DEFAULT`` dicts on for one test: it does not depend on the measured default."""
    from bmp import functional as Fn
    for default in defaults:
        for key in default:
            monkeypatch.setitem(default, key, True)
    return Fn


FUSED, COMPOSED = {"fused": 1, "composed": 0}, {"fused": 0, "composed": 1}


def fused(n):
    return {"fused": n, "composed": 0}


# ---- one step on a table ----
def compare(a, b, tag, tol, names, labels):
    """(out, {operand: gradient}) pairs; a gradient the reference does not have (None) is skipped."""
    close(a[0], b[0], f"{tag}: {labels[0]}", tol=tol)
    for k, nm in zip(names, labels[1:]):
        if b[1][k] is not None:
            close(a[1][k], b[1][k], f"{tag}: {nm}", tol=tol)


def step_against_composed_and_restatement(paths, run, ref, tag, names, labels, forward_only):
    """``run(fused)`` is one step forward and backward in float32, (out, {operand: gradient}); ``ref`` the float64 restatement
    in the same form; ``forward_only`` the calls under ``no_grad`` that must take the kernel and give the same output."""
    fz, tk = took(paths, lambda: run(True))
    assert tk == FUSED, tk
    comp, tk = took(paths, lambda: run(False))
    assert tk == COMPOSED, tk
    compare(fz, comp, f"table {tag} vs composed", 1e-5, names, labels)
    compare(fz, ref, f"table {tag} vs float64", 1e-4, names, labels)
    compare(comp, ref, f"composed {tag} vs float64", 1e-4, names, labels)
    again = run(True)
    assert torch.equal(again[0], fz[0])
    assert all(torch.equal(again[1][k], fz[1][k]) for k in names if fz[1][k] is not None)
    with torch.no_grad():                                # the forward that saves nothing
        for call in forward_only:
            out, tk = took(paths, call)
            assert tk == FUSED and torch.equal(out, fz[0]), tk
    return fz, comp


# ---- through the C ABI ----
def whole_tiles_bit_for_bit(pb, run, label, nonzero, contracted=()):
    """Every table entry a four-block tile at 128 t on a whole-tile batch: ``run(entry, tab)`` calls the family's "tile" or
    "table" entries, forward and backward, and returns its dict of written arrays.  The products run in the same order, so every
    array is bit-identical but those named in ``contracted``, held to 1e-5."""
    from bmp._lib import ptr
    assert pb.mt_row0 is None and not pb.oversized and pb.n_tiles >= 3
    r0 = torch.arange(pb.n_tiles, dtype=torch.int32, device=dev()) * 128
    nb = torch.full((pb.n_tiles,), 4, dtype=torch.int32, device=dev())
    res = {entry: run(entry, tab) for entry, tab in (("tile", ()), ("table", (ptr(r0), ptr(nb), pb.n_rows, 0)))}
    for k, x in res["table"].items():
        assert torch.isfinite(x).all(), k
        print(f"[whole tiles] {label} {k}: max |table - tile| = {(x - res['tile'][k]).abs().max().item():.3e}")
        if k in contracted:
            close(x, res["tile"][k], f"table of whole tiles {label}: {k}", tol=1e-5)
        else:
            assert torch.equal(x, res["tile"][k]), (k, (x - res["tile"][k]).abs().max().item())
    assert all(res["table"][k].abs().max() > 0 for k in nonzero)


def fixed_stride_clears_the_dead_rows(res, live, nonzero, label=None):
    """``res[128]`` and ``res[0]``: the family's written arrays (``nan_rows``) after forward and backward on ``stride_case`` with
    and without the stride.  With it the dead rows are exactly 0 and no NaN is left; the live rows are finite and equal the
    dense-row run, which leaves the dead rows NaN; the canary behind mt_rows stays NaN either way.  The live rows are compared
    bit for bit, or with ``label`` at 1e-5 between the two float32 forms."""
    N = STRIDE_ROWS
    for name, x in res[128].items():
        y = res[0][name]
        assert x.shape[0] == y.shape[0] == N + CANARY_ROWS, name
        assert torch.isnan(x[N:]).all() and torch.isnan(y[N:]).all(), name       # the canary behind mt_rows
        x, y = x[:N], y[:N]
        assert not torch.isnan(x).any(), name
        assert (x[~live] == 0).all(), name
        assert torch.isfinite(x[live]).all(), name
        if label is None:
            assert torch.equal(x[live], y[live]), name
        else:
            close(x[live], y[live], f"fixed stride {label}: live rows of {name} vs dense rows", tol=1e-5)
        assert torch.isnan(y[~live]).all(), name          # (without a stride nothing is written there)
    assert all(res[128][k][:N][live].abs().max() > 0 for k in nonzero)


def bad_tables(r0, nb):
    """The five tables every table entry refuses: a stride that is no multiple of 32 or shorter than a full tile, a missing
    mt_row0 or mt_nblk, no rows."""
    from bmp._lib import ptr
    N = STRIDE_ROWS
    return ((ptr(r0), ptr(nb), N, 96), (ptr(r0), ptr(nb), N, 130), (None, ptr(nb), N, 0), (ptr(r0), None, N, 0), (ptr(r0), ptr(nb), 0, 0))


def refuses_the_bad_tables(r0, nb, *calls):
    """Each ``call(tab)``, a family's forward or backward table entry, fails its argument check on each of ``bad_tables``."""
    for tab in bad_tables(r0, nb):
        for call in calls:
            with pytest.raises(ValueError, match="argument check failed"):
                call(tab)


# ---- encoder level ----
def close_runs(got, want, tag, against):
    """Two ``pair_run`` results: y, g1, g2 and, where both ran backward, every gradient at 1e-5."""
    for k in ("y", "g1", "g2"):
        close(got[k], want[k], f"{tag}: {k}{against}", tol=1e-5)
    if want["grads"]:
        gmax = max(v.abs().max().item() for v in want["grads"].values())
        assert sorted(got["grads"]) == sorted(want["grads"])
        for name, gr in got["grads"].items():
            close(gr, want["grads"][name], f"{tag}: grad {name}{against}", tol=1e-5, floor=1e-3 * gmax)


def encoder_layout_against_per_instance(w, model, paths, tag, dedup, n_cu, took_inst, took_enc=None, backward=True,
                                        atoms=None, atoms_name="atoms", nonzero="graph_conv/message_layers"):
    """The model on the world's pairs per instance and in the encoder layout: the paths taken, y, g1, g2, the loss, every
    gradient and the atom array handed to the co-attention (``atoms()``, read after each run).  (per-instance, encoder)."""
    pb, t, eb, t2 = batches(w, dedup, n_cu)
    inst, tk = took(paths, lambda: pair_run(model, pb, t, backward))
    assert tk == took_inst, tk
    at_inst = atoms() if atoms else None
    enc, tk = took(paths, lambda: pair_run(model, eb, t2, backward))
    assert tk == (took_enc or took_inst), tk
    close_runs(enc, inst, tag, " vs per-instance")
    loss_i, loss_e = model.loss(inst["y"], t).detach().reshape(1), model.loss(enc["y"], t2).detach().reshape(1)
    close(loss_e, loss_i, f"{tag}: loss vs per-instance", tol=1e-5)
    if backward:
        assert any(v.abs().max() > 0 for k, v in enc["grads"].items() if k.startswith(nonzero))
    if atoms:
        at_enc = atoms()
        assert at_enc.pb is eb.pb
        close(atoms_by_molecule(w, at_enc.rows, eb.pb), atoms_by_molecule(w, at_inst.rows, pb), f"{tag}: {atoms_name}", tol=1e-5)
    return inst, enc


def paths_follow_the_switch(monkeypatch, w, model, paths, default, key, layers):
    """With ``default[key]`` on the table batch takes the kernels, off the composed operators, with the same result."""
    pb, t, eb, t2 = batches(w, True, 5)
    res = {}
    for on in (True, False):
        monkeypatch.setitem(default, key, on)
        res[on], tk = took(paths, lambda: pair_run(model, eb, t2))
        assert tk == ({"fused": layers, "composed": 0} if on else {"fused": 0, "composed": layers}), (on, tk)
    close_runs(res[True], res[False], "table kernels vs composed", "")


# ---- the fixed-shape batch ----
def static_eager_step_equals_the_packed_step(model, paths, layers, label, masks=None):
    """Batch k0 holds the store's tallest molecules and batch k1, loaded into the same arrays afterwards, its shortest: rows that
    k0 left behind in a dead block would enter k1's weight gradients.  ``masks`` = (width, drop probability): training mode with
    the dropout masks given, row for row the same in both layouts."""
    from bmp import packed
    from bmp.dp import FlatAdam
    ds, by_size, sizes = static_world()
    B = 8
    assert model.training
    opt = FlatAdam(model, alpha=1e-3)
    sb = packed.StaticPairBatch(ds, B)
    rs = np.random.RandomState(4)
    tall, short = by_size[:2 * B], by_size[-2 * B:]
    assert min(sizes[k] for k in tall) > 64 and max(sizes[k] for k in short) < 31        # 3-4 live blocks, then one
    g = torch.Generator().manual_seed(12)
    for tag, sel in (("k0 tallest", tall), ("k1 shortest", short)):
        i1, i2 = sel[:B], sel[B:]
        lab = rs.randint(0, 2, (B, 1)).astype(np.int32)
        pb, t = packed.pack_from_store_device(ds, [i1, i2], labels=lab)
        sb.load([i1, i2], lab); sb.reset_derived(); sb.emit()
        assert sb.pb.mt_row0 is not None and sb.pb.tile_stride == 128
        mp = msb = None
        if masks:
            d, p_drop = masks
            r0p, r0s = pb.mol_row0.cpu().long(), sb.pb.mol_row0.cpu().long()
            nrows = pb.mol_nrows.cpu().long()
            assert torch.equal(nrows, sb.pb.mol_nrows.cpu().long())
            mp, msb = [], []
            for _ in range(layers):
                k = (torch.rand(pb.n_rows, d, generator=g) >= p_drop).float() / (1.0 - p_drop)
                s = torch.ones(sb.pb.n_rows, d)
                for i in range(2 * B):
                    s[r0s[i]:r0s[i] + nrows[i]] = k[r0p[i]:r0p[i] + nrows[i]]
                mp.append(k.to(dev())); msb.append(s.to(dev()))
            model.graph_conv._dropout_masks = mp
        loss, tk = took(paths, lambda: opt.functional_loss(pb, t=t))
        assert tk == fused(layers), tk
        loss.backward(); opt.collect_grads()
        y_ref, g_ref, l_ref = model.y.detach().clone(), opt.grad.clone(), loss.detach().clone()
        if masks:
            model.graph_conv._dropout_masks = msb
        loss, tk = took(paths, lambda: opt.functional_loss(sb.pb, t=sb.t))
        assert tk == fused(layers), tk
        loss.backward(); opt.collect_grads()
        close(model.y.detach(), y_ref, f"static {label} {tag}: logits", tol=1e-5)
        close(loss.detach().reshape(1), l_ref.reshape(1), f"static {label} {tag}: loss", tol=1e-5)
        close(opt.grad, g_ref, f"static {label} {tag}: flat gradient", tol=1e-5)
        assert g_ref.abs().max() > 0


def fit_runs_in_every_layout(paths, build, label):
    """``fit`` over PairBatches per instance, in the encoder layout with dedup and as replays of one recorded step
    (layout="static"; the short last batch of a pass runs launch by launch): the same losses epoch by epoch at the bound of
    tests/test_trainer.py's layout comparison (different summation orders only), and the same parameters after two passes."""
    from bmp import packed, synth, trainer as Tr
    from bmp.dp import FlatAdam
    store = synth.make_store(40, seed=3, n_lo=4, n_hi=40, n_mean=16)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev())
    rs = np.random.RandomState(1)
    i1, i2 = rs.randint(0, 40, 200), rs.randint(0, 40, 200)
    nat = np.array([m.n for m in store])
    lab = ((nat[i1] + nat[i2]) % 2).astype(np.int32).reshape(-1, 1)
    runs, tk, flat = {}, {}, {}
    for name, kw in (("instance", {}), ("dedup", dict(layout="encoder", dedup=True)), ("static", dict(layout="static"))):
        torch.manual_seed(0)
        model = build().to(dev())
        opt = FlatAdam(model, alpha=2e-3)
        tr = Tr.PairBatches(ds, i1[:144], i2[:144], lab[:144], 32, shuffle=True, seed=2, **kw)
        va = Tr.PairBatches(ds, i1[144:], i2[144:], lab[144:], 32, **kw)
        assert len(tr) == 5 and len(va) == 2
        tr.check_encoder(model)
        runs[name], tk[name] = took(paths, lambda: Tr.fit(model, opt, tr, va, epochs=2))
        flat[name] = opt.flat.detach().clone()
    assert tk["instance"]["composed"] == 0 and tk["instance"]["fused"] > 0, tk
    assert tk["dedup"]["composed"] == 0 and tk["dedup"]["fused"] > 0, tk          # the table kernels, every step
    assert tk["static"]["composed"] == 0 and 0 < tk["static"]["fused"] < tk["instance"]["fused"], tk       # replays
    for name in ("dedup", "static"):
        for a, b in zip(runs["instance"], runs[name]):
            for key in ("main/loss", "validation/main/loss"):
                print(f"[fit] {name} {key}: {b[key]:.7f} vs per-instance {a[key]:.7f}")
                assert abs(a[key] - b[key]) <= 2e-4 * abs(a[key]), (name, key, a[key], b[key])
        close(flat[name], flat["instance"], f"fit {label} {name}: parameters after two passes vs per-instance", tol=1e-4)


def static_recorded_step_replays_on_the_table_kernels(make_model, paths, label):
    """Four batches (tall, short, then mixed) through an eager FlatAdam step and through one recorded step: the recording takes
    the table kernels, a replay runs no Python step, and losses and parameters agree."""
    from bmp import packed
    from bmp.dp import FlatAdam, GraphedTrainStep
    ds, by_size, _sizes = static_world()
    B, steps = 8, 4
    eager, graphed = make_model(), make_model()
    oe, og = FlatAdam(eager, alpha=1e-3), FlatAdam(graphed, alpha=1e-3)
    assert torch.equal(oe.flat, og.flat)
    sb = packed.StaticPairBatch(ds, B)
    stepper = GraphedTrainStep(graphed, og)
    rs = np.random.RandomState(6)
    order = np.concatenate((by_size[:2 * B], by_size[-2 * B:], rs.permutation(48)[:4 * B]))       # tall, short, then mixed
    le, lg = [], []
    for k in range(steps):
        sel = order[2 * B * k:2 * B * (k + 1)]
        i1, i2 = sel[:B], sel[B:]
        lab = rs.randint(0, 2, (B, 1)).astype(np.int32)
        pb, t = packed.pack_from_store_device(ds, [i1, i2], labels=lab)
        loss = oe.functional_loss(pb, t=t); loss.backward(); oe.collect_grads(); oe.step()
        le.append(float(loss.detach()))
        sb.load([i1, i2], lab)
        loss, tk = took(paths, lambda: stepper(sb))
        lg.append(float(loss.detach()))
        assert tk["composed"] == 0, tk                    # the recording took the table kernels, every call of it
        assert (tk["fused"] > 0) == (k == 0), tk          # ... and a replay runs no Python step
    assert len(stepper.graphs) == 1 and og.t == oe.t == steps
    close(torch.tensor(lg), torch.tensor(le), f"recorded {label} step: losses of {steps} steps", tol=1e-4)
    close(og.flat, oe.flat, f"recorded {label} step: parameters after {steps} steps", tol=1e-4)
    assert not np.allclose(le[0], le[-1])
