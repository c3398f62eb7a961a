"""The d = 32 fuse-gate / simple-gate step on a TILE TABLE (csrc/bmp_gate_small_table.hip) and the gated encoders in the encoder
layout, under de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (tests/ggate_ref.py), 1e-5 between two
float32 forms of the same step (test_gpu_static_batch.py, test_gpu_enclayout.py at full size), 1e-4 for parameters after several
replayed steps (test_gpu_static_batch.py).  Every case is a few hundred rows at d = 32.

The hand-made store has the atom counts 31, 32, 33, 63, 64, 95, 96, 127, 2, 5: with one tile per molecule (n_cu = 256) the pad row
falls on the last row of a one-block tile, on the first row of a second block and on row 127 of a full tile; with n_cu = 2 tiles are
shared and a molecule crosses a 32-row block boundary; with n_cu = 1 seven small molecules share one two-block tile."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggate_ref as G                                  # noqa: E402
import ggate32_ref as R                                # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from enc_tables import COUNTS, TABLES, _hand_store     # noqa: E402,F401 (test_gpu_ggdev_enc.py takes them from here)
from parity_util import close                          # noqa: E402
from test_gpu_ops import dev, to_dev                   # noqa: E402

T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 32
KIND = {"fuse": 0, "gate": 1}
_CACHE = {}


def _table(name):
    """(host EncBatch without dedup, its plan) of one of the three tables, its properties asserted."""
    if name not in _CACHE:
        from bmp import enclayout, packed
        if name == "dense":
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


def _dense_adj(pb):
    """(1, 4, N, N) float64 adjacency of the batch's rows from its CSR: adj[0, e, dst, src] = val."""
    N = pb.n_rows
    ptr_, col, val = pb.csr_ptr.numpy(), pb.csr_col.numpy(), pb.csr_val.numpy()
    adj = np.zeros((1, 4, N, N))
    dst = np.repeat(np.arange(N), np.diff(ptr_[:N + 1]))
    adj[0, col & 3, dst, col >> 2] = val
    return adj


def _operands(kind, name):
    """Float64 operands of one step on table ``name`` in the kernel's layouts, drawn once: h, WT, bE, AU, bU, keep, cotangent."""
    key = ("ops", kind, name)
    if key not in _CACHE:
        N = _table(name).pb_enc.n_rows
        g = torch.Generator().manual_seed(100 + KIND[kind])
        r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
        nu = (3 if kind == "fuse" else 1) * D
        keep = ((torch.rand(N, D, generator=g) >= 0.3).double() / 0.7) if kind == "fuse" else None
        _CACHE[key] = dict(h=r(N, D), WT=0.5 * r(4 * D, D) / D ** 0.5, bE=0.3 * r(4, D), AU=r(2 * D, nu) / (2 * D) ** 0.5,
                           bU=0.3 * r(nu), keep=keep, c=r(N, D))
    return _CACHE[key]


NAMES = ("h", "WT", "bE", "AU", "bU")


def _restatement(kind, name):
    """tests/ggate_ref.py's forward for ONE step on the table's rows as one dense 'molecule' of N positions; the leaves are the
    kernel-layout operands, so their gradients come out in the kernel's layouts.  (hout, {operand: gradient})."""
    key = ("ref", kind, name)
    if key not in _CACHE:
        o = _operands(kind, name)
        q = {k: o[k].clone().requires_grad_() for k in NAMES}
        N = o["h"].shape[0]
        p = {"embed/W": q["h"],
             "message_layers/0/W": q["WT"].view(4, D, D).permute(2, 0, 1).reshape(4 * D, D),       # feature 4 c + e <- WT[e d + k, c]
             "message_layers/0/b": q["bE"].t().reshape(4 * D)}
        if kind == "fuse":
            for k in (1, 2, 3):
                p[f"update_layer{k}/W"] = q["AU"][:, (k - 1) * D:k * D].t()
                p[f"update_layer{k}/b"] = q["bU"][(k - 1) * D:k * D]
        else:
            p["gate_layer/0/W"], p["gate_layer/0/b"] = q["AU"].t(), q["bU"]
        z = torch.zeros
        p.update({"i_layers/0/W": z(4, 2 * D, dtype=torch.float64), "i_layers/0/b": z(4, dtype=torch.float64),
                  "j_layers/0/W": z(4, D, dtype=torch.float64), "j_layers/0/b": z(4, dtype=torch.float64)})
        keep = None if o["keep"] is None else [o["keep"][None]]
        _g, h = G.forward(kind, p, np.arange(N)[None], _dense_adj(_table(name).pb_enc), 1, keep=keep)
        (h[0] * o["c"]).sum().backward()
        _CACHE[key] = (h[0].detach(), {k: q[k].grad for k in NAMES})
    return _CACHE[key]


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.GATE_PATHS)
    out = fn()
    return out, {k: Fn.GATE_PATHS[k] - before[k] for k in before}


def _run_step(kind, name, pb, fused):
    """One step forward and backward in float32 on the device: (hout, {operand: gradient})."""
    from bmp import functional as Fn
    o = _operands(kind, name)
    q = {k: o[k].float().to(dev()).requires_grad_() for k in NAMES}
    keep = None if o["keep"] is None else o["keep"].float().to(dev())
    if fused:
        hout = Fn.GateStepFn.apply(q["h"], q["WT"], q["bE"], q["AU"], q["bU"], keep, pb, KIND[kind])
    else:
        hout = Fn.gate_step(q["h"], q["WT"], q["bE"], q["AU"], q["bU"], KIND[kind], keep, pb, fused=False)
    (hout * o["c"].float().to(dev())).sum().backward()
    return hout.detach(), {k: q[k].grad for k in NAMES}


def _compare(a, b, tag, tol):
    close(a[0], b[0], f"{tag}: hout", tol=tol)
    for k, nm in zip(NAMES, ("dh", "dWT", "dbE", "dAU", "dbU")):
        close(a[1][k], b[1][k], f"{tag}: {nm}", tol=tol)


@pytest.mark.parametrize("name", ["own", "shared", "seven"])
@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_table_step_against_composed_and_restatement(kind, name):
    from bmp import functional as Fn
    pb = to_dev(_table(name).pb_enc)
    ref = _restatement(kind, name)
    fused, took = _took(lambda: _run_step(kind, name, pb, True))
    assert took == {"fused": 1, "composed": 0}, took
    comp, took = _took(lambda: _run_step(kind, name, pb, False))
    assert took == {"fused": 0, "composed": 1}, took
    _compare(fused, comp, f"table {name} {kind} vs composed", 1e-5)
    _compare(fused, ref, f"table {name} {kind} vs float64", 1e-4)
    _compare(comp, ref, f"composed {name} {kind} vs float64", 1e-4)
    again = _run_step(kind, name, pb, True)
    assert torch.equal(again[0], fused[0]) and all(torch.equal(again[1][k], fused[1][k]) for k in NAMES)
    o = _operands(kind, name)
    with torch.no_grad():                                # the forward that saves nothing
        args = [o[k].float().to(dev()) for k in NAMES]
        keep = None if o["keep"] is None else o["keep"].float().to(dev())
        h0, took = _took(lambda: Fn.GateStepFn.apply(*args, keep, pb, KIND[kind]))
    assert took == {"fused": 1, "composed": 0} and torch.equal(h0, fused[0])


def _stride_case():
    """Three tiles at the fixed stride 128 with 1, 2 and 3 live blocks: molecules of 20, 40 and 70 atoms (chains, cycling bond
    types) and their pad rows.  (csr, csrT, mt_row0, mt_nblk, live-row mask)."""
    ns, N = [20, 40, 70], 384
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
        i32 = lambda a: T(np.ascontiguousarray(a).astype(np.int32)).to(dev())
        return i32(p_), i32((minor[order] << 2) | typ[order]), torch.ones(len(order), device=dev())

    nblk = [(n + 1 + 31) // 32 for n in ns]
    assert nblk == [1, 2, 3]
    live = np.zeros(N, dtype=bool)
    for t, k in enumerate(nblk):
        live[128 * t:128 * t + 32 * k] = True
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev())
    return build(dst, src), build(src, dst), i32([0, 128, 256]), i32(nblk), torch.from_numpy(live).to(dev())


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_fixed_stride_clears_the_dead_rows(kind):
    """Through the C ABI: every output prefilled with NaN, the inputs' dead rows NaN too (never read).  With tile_stride = 128 the
    rows of the dead blocks are exactly 0 after forward and backward; the live rows are finite and bit-equal to tile_stride = 0."""
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    from bmp.functional import pack_k4
    L = _lib.lib()
    (cp, cc, cv), (tp, tc, tv), r0, nb, live = _stride_case()
    N, nu, k = 384, (3 if kind == "fuse" else 1) * D, KIND[kind]
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    nan_dead = lambda x: torch.where(live[:, None], x, torch.full_like(x, float("nan")))
    h, dhout = nan_dead(rnd(N, D)), nan_dead(rnd(N, D))
    keep = nan_dead((torch.rand(N, D, generator=g) >= 0.3).float().to(dev()) / 0.7) if kind == "fuse" else None
    WT, bE, AU, bU = 0.1 * rnd(4 * D, D), 0.3 * rnd(4, D), 0.1 * rnd(2 * D, nu), 0.3 * rnd(nu)
    WTp, AUp, Wnp, Unp = pack_k4(WT), pack_k4(AU), pack_k4(WT.t()), pack_k4(AU.t())
    res = {}
    for stride in (128, 0):
        nan = lambda *s: torch.full(s, float("nan"), device=dev())
        m, act, hout, dh, gda = nan(N, D), nan(N, nu), nan(N, D), nan(N, D), nan(N, 4 * D + nu)
        check(L.bmp_ggnn_gate_step_small_table_fwd(k, ptr(h), 3, D, ptr(cp), ptr(cc), ptr(cv), ptr(WTp), ptr(bE), ptr(AUp), ptr(bU),
                                                   ptr(keep), ptr(m), ptr(act), ptr(hout), ptr(r0), ptr(nb), N, stride, stream()),
              "bmp_ggnn_gate_step_small_table_fwd")
        check(L.bmp_ggnn_gate_step_small_table_bwd(k, ptr(dhout), ptr(h), ptr(m), ptr(act), ptr(keep), 3, D, ptr(tp), ptr(tc), ptr(tv),
                                                   ptr(Wnp), ptr(Unp), ptr(dh), ptr(gda), ptr(r0), ptr(nb), N, stride, stream()),
              "bmp_ggnn_gate_step_small_table_bwd")
        torch.cuda.synchronize()
        res[stride] = dict(m=m, act=act, hout=hout, dh=dh, gda=gda)
    for name, x in res[128].items():
        assert (x[~live] == 0).all(), name
        assert torch.isfinite(x[live]).all(), name
        assert torch.equal(x[live], res[0][name][live]), name
        assert torch.isnan(res[0][name][~live]).all(), name          # (without a stride nothing is written there)
    assert res[128]["hout"][live].abs().max() > 0 and res[128]["gda"][live].abs().max() > 0
    # the table entries refuse a stride that is no multiple of 32 or shorter than a full tile, and a missing table
    for bad in (96, 130):
        with pytest.raises(ValueError, match="argument check failed"):
            check(L.bmp_ggnn_gate_step_small_table_fwd(k, ptr(h), 3, D, ptr(cp), ptr(cc), ptr(cv), ptr(WTp), ptr(bE), ptr(AUp), ptr(bU),
                                                       ptr(keep), None, None, ptr(res[0]["hout"]), ptr(r0), ptr(nb), N, bad, stream()),
                  "bmp_ggnn_gate_step_small_table_fwd")
    with pytest.raises(ValueError, match="argument check failed"):
        check(L.bmp_ggnn_gate_step_small_table_fwd(k, ptr(h), 3, D, ptr(cp), ptr(cc), ptr(cv), ptr(WTp), ptr(bE), ptr(AUp), ptr(bU),
                                                   ptr(keep), None, None, ptr(res[0]["hout"]), None, ptr(nb), N, 0, stream()),
              "bmp_ggnn_gate_step_small_table_fwd")


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_table_tile_with_more_entries_than_the_staged_csr(kind):
    """One four-block table tile whose CSR does not fit the staging in LDS: both directions gather from global memory."""
    pb = to_dev(_table("dense").pb_enc)
    fused, took = _took(lambda: _run_step(kind, "dense", pb, True))
    assert took == {"fused": 1, "composed": 0}, took
    _compare(fused, _run_step(kind, "dense", pb, False), f"dense table tile {kind} vs composed", 1e-5)


# ---- encoder level: the 9-molecule, 13-pair heavy-repetition set of test_gpu_enclayout.py ----
I1 = np.array([0, 1, 2, 0, 3, 3, 8, 1, 0, 5, 5, 2, 6]); I2 = np.array([1, 0, 0, 0, 4, 3, 1, 8, 7, 5, 2, 2, 6])
LAB = (np.arange(13).reshape(-1, 1) % 2).astype(np.int32)
LAYERS = 3


def _world():
    if "world" not in _CACHE:
        from bmp import packed, synth
        store = synth.make_store(9, seed=31, n_lo=2, n_hi=60, n_mean=16)
        ms = packed.MolStore(store)
        _CACHE["world"] = (store, ms, packed.DeviceMolStore(ms, dev()))
    return _CACHE["world"]


def _pair_params(kind, attn, d=D):
    dr = O._Draw(21, torch.float64, 0.1)
    if attn == "nie":
        O.init_nie(dr, "attn/", d, d, 8)
    O.init_mlp(dr, "mlp/", 2 * d, 1, (32, 16))
    p = dict(dr.p)
    p.update(G.make_params(kind, 50 + KIND[kind], d, d, LAYERS, False, prefix="graph_conv/"))
    return p


def _pair_reference(kind, attn):
    """The float64 restatement of the pair model on the dense arrays, evaluation mode: dict(y, g1, g2, grads)."""
    key = ("pair", kind, attn)
    if key not in _CACHE:
        from bmp import synth
        store = _world()[0]
        q = {k: v.clone().requires_grad_() for k, v in _pair_params(kind, attn).items()}
        out = [G.forward(kind, q, *synth.concat_mols([store[k] for k in idx]), LAYERS, tying=False, prefix="graph_conv/")
               for idx in (I1, I2)]
        g1, g2 = out[0][0], out[1][0]
        if attn == "nie":
            g1, g2 = O.nie_coattention(q, out[0][1], out[1][1], "tanh", prefix="attn/")
        y = O.mlp_forward(q, torch.cat((g1, g2), dim=-1), 2)
        names = sorted(q)
        gr = torch.autograd.grad(O.sigmoid_cross_entropy(y, T(LAB)), [q[n] for n in names], allow_unused=True)
        _CACHE[key] = dict(y=y.detach(), g1=g1.detach(), g2=g2.detach(),
                           grads={n: (x if x is not None else torch.zeros_like(q[n])) for n, x in zip(names, gr)})
    return _CACHE[key]


def _pair_model(kind, attn, d=D):
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    model = build_pair_predictor(encoder="ggnn-" + kind, hidden_dim=d, out_dim=d, n_layers=LAYERS, weight_tying=False, attn=attn).to(dev())
    load_param_dict(model, _pair_params(kind, attn, d))
    return model


def _pair_run(model, batch, t, backward=True):
    from bmp.snapshot import grad_dict
    model.zero_grad()
    y = model(batch)
    if backward:
        model.loss(y, t).backward()
    return dict(y=y.detach(), g1=model.g1.detach(), g2=model.g2.detach(), grads=grad_dict(model) if backward else {})


def _batches(dedup, n_cu):
    from bmp import enclayout, packed
    ds = _world()[2]
    pb, t = packed.pack_from_store_device(ds, [I1, I2], labels=LAB)
    eb, t2 = enclayout.encode_from_store_device(ds, [I1, I2], labels=LAB, dedup=dedup, n_cu=n_cu)
    assert eb.n_encoded == (9 if dedup else 26)
    nb = eb.pb_enc.mt_nblk.cpu().numpy()
    assert nb.min() >= 1 and nb.max() <= 4 and (n_cu != 5 or nb.max() >= 2)
    return pb, t, eb, t2


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
def test_gate_encoder_trains_in_the_encoder_layout(attn, dedup, n_cu):
    pb, t, eb, t2 = _batches(dedup, n_cu)
    model = _pair_model("gate", attn)
    assert model.training
    inst, took = _took(lambda: _pair_run(model, pb, t))
    assert took == {"fused": LAYERS, "composed": 0}, took
    enc, took = _took(lambda: _pair_run(model, eb, t2))
    assert took == {"fused": LAYERS, "composed": 0}, took
    ref = _pair_reference("gate", attn)
    tag = f"gate attn={attn} dedup={dedup} n_cu={n_cu}"
    for k in ("y", "g1", "g2"):
        close(enc[k], inst[k], f"{tag}: {k} vs per-instance", tol=1e-5)
        close(enc[k], ref[k], f"{tag}: {k} vs float64")
    gmax = max(v.abs().max().item() for v in inst["grads"].values())
    assert sorted(enc["grads"]) == sorted(ref["grads"])
    for name, gr in enc["grads"].items():
        # (1e-3 of the largest gradient as the floor of a parameter's scale: test_gpu_enclayout.py at full size)
        close(gr, inst["grads"][name], f"{tag}: grad {name} vs per-instance", tol=1e-5, floor=1e-3 * gmax)
        want = ref["grads"][name]
        floor = 1e-6                                     # the floors of test_gpu_enclayout.py's oracle comparison
        if name == "attn/energy_layer/b":
            floor = ref["grads"]["attn/energy_layer/V1"].abs().max().item()
        if name.startswith("attn/energy_layers"):
            floor = 1e-4 * max(v.abs().max().item() for k, v in ref["grads"].items() if k.startswith("attn/"))
        close(gr, want, f"{tag}: grad {name} vs float64", floor=floor)


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
def test_fuse_encoder_evaluates_in_the_encoder_layout_and_refuses_to_train_there(attn, dedup, n_cu):
    from bmp import ggnn_gate
    pb, t, eb, t2 = _batches(dedup, n_cu)
    model = _pair_model("fuse", attn).eval()
    with torch.no_grad():
        inst, took = _took(lambda: _pair_run(model, pb, t, backward=False))
        assert took == {"fused": LAYERS, "composed": 0}, took
        enc, took = _took(lambda: _pair_run(model, eb, t2, backward=False))
        assert took == {"fused": LAYERS, "composed": 0}, took
    ref = _pair_reference("fuse", attn)
    tag = f"fuse attn={attn} dedup={dedup} n_cu={n_cu}"
    for k in ("y", "g1", "g2"):
        close(enc[k], inst[k], f"{tag}: {k} vs per-instance", tol=1e-5)
        close(enc[k], ref[k], f"{tag}: {k} vs float64")
    model.train()
    with pytest.raises(NotImplementedError) as e:
        model(eb)
    assert str(e.value) == "encode_rows: " + ggnn_gate.FUSE_TRAIN_LAYOUT_REASON


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_width_64_on_a_table_batch_stays_composed(kind):
    """The d = 64 / 128 kernels take no table: the encoder layout runs the composed operators there, with the per-instance
    result."""
    pb, t, eb, t2 = _batches(True, 5)
    model = _pair_model(kind, None, d=64).eval()
    inst, took = _took(lambda: _pair_run(model, pb, t))
    assert took == {"fused": LAYERS, "composed": 0}, took
    enc, took = _took(lambda: _pair_run(model, eb, t2))
    assert took == {"fused": 0, "composed": LAYERS}, took
    for k in ("y", "g1", "g2"):
        close(enc[k], inst[k], f"d = 64 {kind} table batch: {k} vs per-instance", tol=1e-5)
    gmax = max(v.abs().max().item() for v in inst["grads"].values())
    for name, gr in enc["grads"].items():
        close(gr, inst["grads"][name], f"d = 64 {kind} table batch: grad {name} vs per-instance", tol=1e-5, floor=1e-3 * gmax)


# ---- the fixed-shape batch ----
def _static_world():
    if "static" not in _CACHE:
        from bmp import packed, synth
        store = (synth.make_store(16, seed=3, n_lo=70, n_hi=120, n_mean=95) + synth.make_store(16, seed=4, n_lo=3, n_hi=28, n_mean=12)
                 + synth.make_store(16, seed=5, n_lo=20, n_hi=70, n_mean=40))          # sixteen tall, sixteen short, sixteen between
        ds = packed.DeviceMolStore(packed.MolStore(store), dev())
        by_size = np.argsort([-m.n for m in store], kind="stable")
        _CACHE["static"] = (ds, by_size, [m.n for m in store])
    return _CACHE["static"]


def _static_model(kind):
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.ggnn_gate import FuseGGNN, GateGGNN
    torch.manual_seed(5)
    enc = (FuseGGNN if kind == "fuse" else GateGGNN)(out_dim=16, hidden_dim=D, n_layers=3, weight_tying=False)
    return GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev())


def test_static_batch_eager_fuse_step_equals_the_packed_step():
    """Batch k0 holds the store's tallest molecules and batch k1, loaded into the same arrays afterwards, its shortest: rows that
    k0 left behind in a dead block would enter k1's weight gradients.  Training mode with the masks given, row for row the same
    in both layouts."""
    from bmp import functional as Fn, packed
    from bmp.dp import FlatAdam
    ds, by_size, sizes = _static_world()
    B = 8
    model = _static_model("fuse")
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
        r0p, r0s = pb.mol_row0.cpu().long(), sb.pb.mol_row0.cpu().long()
        nrows = pb.mol_nrows.cpu().long()
        assert torch.equal(nrows, sb.pb.mol_nrows.cpu().long())
        mp, msb = [], []
        for _ in range(3):
            k = (torch.rand(pb.n_rows, D, generator=g) >= 0.05).float() / 0.95
            s = torch.ones(sb.pb.n_rows, D)
            for i in range(2 * B):
                s[r0s[i]:r0s[i] + nrows[i]] = k[r0p[i]:r0p[i] + nrows[i]]
            mp.append(k.to(dev())); msb.append(s.to(dev()))
        model.graph_conv._dropout_masks = mp
        loss = opt.functional_loss(pb, t=t); loss.backward(); opt.collect_grads()
        y_ref, g_ref, l_ref = model.y.detach().clone(), opt.grad.clone(), loss.detach().clone()
        model.graph_conv._dropout_masks = msb
        before = dict(Fn.GATE_PATHS)
        loss = opt.functional_loss(sb.pb, t=sb.t); loss.backward(); opt.collect_grads()
        assert Fn.GATE_PATHS["fused"] - before["fused"] == 3 and Fn.GATE_PATHS["composed"] == before["composed"]
        close(model.y.detach(), y_ref, f"static fuse {tag}: logits", tol=1e-5)
        close(loss.detach().reshape(1), l_ref.reshape(1), f"static fuse {tag}: loss", tol=1e-5)
        close(opt.grad, g_ref, f"static fuse {tag}: flat gradient", tol=1e-5)


def test_static_batch_recorded_gate_step_replays_on_the_table_kernels():
    from bmp import functional as Fn, packed
    from bmp.dp import FlatAdam, GraphedTrainStep
    ds, by_size, _sizes = _static_world()
    B, steps = 8, 4
    eager, graphed = _static_model("gate"), _static_model("gate")
    oe, og = FlatAdam(eager, alpha=1e-3), FlatAdam(graphed, alpha=1e-3)
    assert torch.equal(oe.flat, og.flat)
    sb = packed.StaticPairBatch(ds, B)
    stepper = GraphedTrainStep(graphed, og)
    rs = np.random.RandomState(6)
    order = np.concatenate((by_size[:2 * B], by_size[-2 * B:], rs.permutation(48)[:4 * B]))       # tall, short, then mixed
    le, lg = [], []
    composed = None
    for k in range(steps):
        sel = order[2 * B * k:2 * B * (k + 1)]
        i1, i2 = sel[:B], sel[B:]
        lab = rs.randint(0, 2, (B, 1)).astype(np.int32)
        pb, t = packed.pack_from_store_device(ds, [i1, i2], labels=lab)
        loss = oe.functional_loss(pb, t=t); loss.backward(); oe.collect_grads(); oe.step()
        le.append(float(loss.detach()))
        sb.load([i1, i2], lab)
        if composed is None:
            composed = Fn.GATE_PATHS["composed"]
        lg.append(float(stepper(sb).detach()))
    assert Fn.GATE_PATHS["composed"] == composed                     # the recording took the table kernels
    assert len(stepper.graphs) == 1 and og.t == oe.t == steps
    close(torch.tensor(lg), torch.tensor(le), f"recorded gate step: losses of {steps} steps", tol=1e-4)
    close(og.flat, oe.flat, f"recorded gate step: parameters after {steps} steps", tol=1e-4)
    assert not np.allclose(le[0], le[-1])
