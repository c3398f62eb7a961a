"""The self-loop GGNN step on a TILE TABLE (csrc/bmp_loop_table.hip) and the encoders of bmp/ggnn_dev.py in the encoder layout,
under de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (tests/ggdev_ref.py), 1e-5 between two
float32 forms of the same step, 1e-4 for parameters after several replayed steps (test_gpu_static_batch.py).  The store and the
three tables are tests/test_gpu_ggate_enc.py's (their properties: tests/test_ggdev_enc_build.py); every case is under 800 rows at
d = 64, one repeats at d = 128.  The tests that go through ``loop_step`` force ``LOOP_TABLE_DEFAULT`` on: they do not depend on
the measured default."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggdev_ref as R                                  # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from parity_util import close                          # noqa: E402
from test_gpu_ops import dev, to_dev                   # noqa: E402
from test_gpu_ggate_enc import COUNTS, _dense_adj, _hand_store, _static_world, _table      # noqa: E402

T = torch.from_numpy
NAMES = ("h", "WT", "bE", "WsT", "bs", "AT", "UcT", "b")
GRADS = ("dh", "dWT", "dbE", "dWsT", "dbs", "dAT", "dUcT", "db")
LAYERS = 3
_CACHE = {}


@pytest.fixture
def table_on(monkeypatch):
    from bmp import functional as Fn
    for d in (64, 128):
        monkeypatch.setitem(Fn.LOOP_TABLE_DEFAULT, d, True)
    return Fn


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.LOOP_PATHS)
    out = fn()
    return out, {k: Fn.LOOP_PATHS[k] - before[k] for k in before}


# ---- one step on the three tables ----
def _operands(name, d):
    """Float64 operands of one step on table ``name`` in the kernel's layouts, drawn once, and the cotangent."""
    key = ("ops", name, d)
    if key not in _CACHE:
        N = _table(name).pb_enc.n_rows
        g = torch.Generator().manual_seed(300 + d)
        r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
        _CACHE[key] = dict(h=r(N, d), WT=0.5 * r(4 * d, d) / d ** 0.5, bE=0.3 * r(4, d), WsT=0.5 * r(d, d) / d ** 0.5, bs=0.3 * r(d),
                           AT=r(2 * d, 3 * d) / (2 * d) ** 0.5, UcT=r(d, d) / d ** 0.5, b=0.3 * r(3 * d), c=r(N, d))
    return _CACHE[key]


def _restatement(name, d, first):
    """tests/ggdev_ref.py's step (its message, self loop and stateful GRU, op for op) on the table's rows as one dense 'molecule'
    of N positions; the leaves are the kernel-layout operands, so their gradients come out in the kernel's layouts.  A later call
    takes h as the GRU's state: with the state folded into the h-part (GRU.kernel_weights) U_r = U_z = 0 and U = UcT^T."""
    key = ("ref", name, d, first)
    if key not in _CACHE:
        o = _operands(name, d)
        q = {k: o[k].clone().requires_grad_() for k in NAMES}
        N = o["h"].shape[0]
        adj = _dense_adj(_table(name).pb_enc)
        A = q["AT"].t()
        z = lambda *s: torch.zeros(*s, dtype=torch.float64)
        p = {"embed/W": q["h"],
             "message_layers/0/W": q["WT"].view(4, d, d).permute(2, 0, 1).reshape(4 * d, d),       # feature 4 c + e <- WT[e d + k, c]
             "message_layers/0/b": q["bE"].t().reshape(4 * d),
             "message_self_loop_layers/0/W": q["WsT"].t(), "message_self_loop_layers/0/b": q["bs"],
             "update_layer/W_r/W": A[:d], "update_layer/W_r/b": q["b"][:d], "update_layer/W_z/W": A[d:2 * d],
             "update_layer/W_z/b": q["b"][d:2 * d], "update_layer/W/W": A[2 * d:], "update_layer/W/b": q["b"][2 * d:],
             "update_layer/U_r/W": z(d, d), "update_layer/U_r/b": z(d), "update_layer/U_z/W": z(d, d), "update_layer/U_z/b": z(d),
             "update_layer/U/W": q["UcT"].t(), "update_layer/U/b": z(d),
             "i_layers/0/W": z(4, 2 * d), "i_layers/0/b": z(4), "j_layers/0/W": z(4, d), "j_layers/0/b": z(4)}
        if first:
            _g, hs, _gs = R.forward("loop", p, np.arange(N)[None], adj, 1)
            out = hs[0][0]
        else:                                            # the loop body of ggdev_ref.forward with s = h
            h = q["h"][None]
            m = O.ggnn_message(h, torch.as_tensor(adj), p["message_layers/0/W"], p["message_layers/0/b"])
            m = m + O.linear(h, p["message_self_loop_layers/0/W"], p["message_self_loop_layers/0/b"])
            out = O.stateful_gru(p, "update_layer", torch.cat((h[0], m[0]), dim=1), h[0])
        (out * o["c"]).sum().backward()
        _CACHE[key] = (out.detach(), {k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])) for k in NAMES})
    return _CACHE[key]


def _run_step(name, d, first, pb, fused):
    """One step forward and backward in float32 on the device: (hout, {operand: gradient})."""
    from bmp import functional as Fn
    o = _operands(name, d)
    q = {k: o[k].float().to(dev()).requires_grad_() for k in NAMES}
    if fused:
        hout = Fn.LoopStepFn.apply(*(q[k] for k in NAMES), pb, first)
    else:
        hout = Fn.loop_step(*(q[k] for k in NAMES), first, pb, fused=False)
    (hout * o["c"].float().to(dev())).sum().backward()
    return hout.detach(), {k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])) for k in NAMES}


def _compare(a, b, tag, tol):
    close(a[0], b[0], f"{tag}: hout", tol=tol)
    for k, nm in zip(NAMES, GRADS):
        close(a[1][k], b[1][k], f"{tag}: {nm}", tol=tol)


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("name,d", [("own", 64), ("shared", 64), ("seven", 64), ("own", 128)])
def test_table_step_against_composed_and_restatement(name, d, first, table_on):
    Fn = table_on
    pb = to_dev(_table(name).pb_enc)
    r0, nb = pb.mt_row0.cpu().numpy(), pb.mt_nblk.cpu().numpy()
    cover = np.zeros(pb.n_rows, dtype=int)
    for a, k in zip(r0, nb):
        cover[a:a + 32 * k] += 1
    assert (cover == 1).all() and pb.n_rows < 800        # the table's tiles abut and hold every row once
    ref = _restatement(name, d, first)
    fused, took = _took(lambda: _run_step(name, d, first, pb, True))
    assert took == {"fused": 1, "composed": 0}, took
    comp, took = _took(lambda: _run_step(name, d, first, pb, False))
    assert took == {"fused": 0, "composed": 1}, took
    tag = f"{name} d={d} first={first}"
    _compare(fused, comp, f"table {tag} vs composed", 1e-5)
    _compare(fused, ref, f"table {tag} vs float64", 1e-4)
    _compare(comp, ref, f"composed {tag} vs float64", 1e-4)
    again = _run_step(name, d, first, pb, True)
    assert torch.equal(again[0], fused[0]) and all(torch.equal(again[1][k], fused[1][k]) for k in NAMES)
    o = _operands(name, d)
    with torch.no_grad():                                # forward-only evaluation: null m / rz / c
        args = [o[k].float().to(dev()) for k in NAMES]
        h0, took = _took(lambda: Fn.LoopStepFn.apply(*args, pb, first))
        assert took == {"fused": 1, "composed": 0} and torch.equal(h0, fused[0])
        h1, took = _took(lambda: Fn.loop_step(*args, first, pb))          # ... and what loop_step picks with the switch on
        assert took == {"fused": 1, "composed": 0} and torch.equal(h1, fused[0])


# ---- through the C ABI ----
def _weights(d, seed):
    from bmp.functional import pack_k4
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    WT, WsT, AT, UcT = 0.5 * rnd(4 * d, d) / d ** 0.5, 0.5 * rnd(d, d) / d ** 0.5, rnd(2 * d, 3 * d) / (2 * d) ** 0.5, rnd(d, d) / d ** 0.5
    return dict(WTp=pack_k4(WT), bE=0.3 * rnd(4, d), WsTp=pack_k4(WsT), bs=0.3 * rnd(d), ATp=pack_k4(AT), UcTp=pack_k4(UcT),
                b=0.3 * rnd(3 * d), Wnp=pack_k4(WT.t()), Wsp=pack_k4(WsT.t()), Anp=pack_k4(AT.t()), Ucp=pack_k4(UcT.t()))


def _abi_fwd(entry, first, d, n_tiles, h, csr, W, m, rz, c, hout, tab=()):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    name = f"bmp_ggnn_loop_step_{entry}_fwd"
    check(getattr(_lib.lib(), name)(ptr(h), n_tiles, d, int(first), ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ptr(W["WTp"]), ptr(W["bE"]),
                                    ptr(W["WsTp"]), ptr(W["bs"]), ptr(W["ATp"]), ptr(W["UcTp"]), ptr(W["b"]), ptr(m), ptr(rz), ptr(c),
                                    ptr(hout), *tab, stream()), name)


def _abi_bwd(entry, first, d, n_tiles, dhout, h, rz, c, csrT, W, dh, gda, rh, tab=()):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    name = f"bmp_ggnn_loop_step_{entry}_bwd"
    check(getattr(_lib.lib(), name)(ptr(dhout), ptr(h), ptr(rz), ptr(c), n_tiles, d, int(first), ptr(csrT[0]), ptr(csrT[1]),
                                    ptr(csrT[2]), ptr(W["Wnp"]), ptr(W["Wsp"]), ptr(W["Anp"]), ptr(W["Ucp"]), ptr(dh), ptr(gda), ptr(rh),
                                    *tab, stream()), name)


# (d, first, array) whose last expression the compiler contracts otherwise in the table instance than in the whole-tile one:
# out = z c + (1 - z) h of the later-call forward.  With c = tanh = 1 - t the whole-tile instances multiply z by the rounded c,
# the table instances take z c as fma(-t, z, z) (the device assembly of both was read: 16 subtractions fewer per lane), one
# rounding apart (2.4e-7) at both widths; z (in rz), c, h and every other array of both directions are bit-identical.  Held to
# 1e-5, the tolerance between two float32 forms.
CONTRACTED = {(64, False, "hout"), (128, False, "hout")}


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("d", [64, 128])
def test_table_of_whole_tiles_is_the_whole_tile_kernel_bit_for_bit(d, first):
    """Every table entry a four-block tile at 128 t, on the whole-tile batch of tests/ggdev_ref.py's "fixture" (three tiles, all
    four bond types): the products run in the same order, so every written array is bit-identical."""
    from bmp._lib import ptr
    pb = to_dev(R.data("fixture")["pb"])
    assert pb.mt_row0 is None and not pb.oversized and pb.n_tiles >= 3
    N, nt = pb.n_rows, pb.n_tiles
    csr, csrT = (pb.csr_ptr, pb.csr_col, pb.csr_val), (pb.csrT_ptr, pb.csrT_col, pb.csrT_val)
    W = _weights(d, 40 + d)
    g = torch.Generator().manual_seed(41)
    h, dhout = torch.randn(N, d, generator=g).to(dev()), torch.randn(N, d, generator=g).to(dev())
    r0 = torch.arange(nt, dtype=torch.int32, device=dev()) * 128
    nb = torch.full((nt,), 4, dtype=torch.int32, device=dev())
    res = {}
    for entry, tab in (("tile", ()), ("table", (ptr(r0), ptr(nb), N, 0))):
        z = lambda n: torch.zeros(N, n, device=dev())
        m, rz, c, hout, dh, gda, rh = z(d), z(2 * d), z(d), z(d), z(d), z(8 * d), (None if first else z(d))
        _abi_fwd(entry, first, d, nt, h, csr, W, m, rz, c, hout, tab)
        _abi_bwd(entry, first, d, nt, dhout, h, rz, c, csrT, W, dh, gda, rh, tab)
        torch.cuda.synchronize()
        res[entry] = dict(m=m, rz=rz, c=c, hout=hout, dh=dh, gda=gda, rh=rh if rh is not None else z(1))
    for k, x in res["table"].items():
        assert torch.isfinite(x).all(), k
        print(f"[whole tiles] d={d} first={first} {k}: max |table - tile| = {(x - res['tile'][k]).abs().max().item():.3e}")
        if (d, first, k) in CONTRACTED:
            close(x, res["tile"][k], f"table of whole tiles d={d} first={first}: {k}", tol=1e-5)
        else:
            assert torch.equal(x, res["tile"][k]), (k, (x - res["tile"][k]).abs().max().item())
    assert res["table"]["hout"].abs().max() > 0 and res["table"]["gda"].abs().max() > 0


def _stride_case():
    """Three tiles at the fixed stride 128 with 1, 3 and 4 live blocks: molecules of 20, 70 and 120 atoms (chains, cycling bond
    types) and their pad rows.  (csr, csrT, mt_row0, mt_nblk, live-row mask); N = 384."""
    ns, N = [20, 70, 120], 384
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
    assert nblk == [1, 3, 4]
    live = np.zeros(N, dtype=bool)
    for t, k in enumerate(nblk):
        live[128 * t:128 * t + 32 * k] = True
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev())
    return build(dst, src), build(src, dst), i32([0, 128, 256]), i32(nblk), torch.from_numpy(live).to(dev())


@pytest.mark.parametrize("first", [True, False])
def test_fixed_stride_clears_the_dead_rows(first):
    """Through the C ABI at d = 64: every output prefilled with NaN, the dead rows of h, dhout, rz and c NaN too (never read), and a
    128-row NaN canary behind mt_rows in every written array.  With tile_stride = 128 the rows of the dead blocks are exactly 0
    after forward and backward and the live rows finite and bit-equal to tile_stride = 0, which leaves the dead rows NaN; the
    canary stays NaN either way."""
    from bmp._lib import ptr
    d, N, C = 64, 384, 128
    csr, csrT, r0, nb, live = _stride_case()
    W = _weights(d, 77)
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    nan_dead = lambda x: torch.where(live[:, None], x, torch.full_like(x, float("nan")))
    h, dhout = nan_dead(rnd(N, d)), nan_dead(rnd(N, d))
    res = {}
    for stride in (128, 0):
        nan = lambda n: torch.full((N + C, n), float("nan"), device=dev())
        m, rz, c, hout, dh, gda = nan(d), nan(2 * d), nan(d), nan(d), nan(d), nan(8 * d)
        rh = None if first else nan(d)
        tab = (ptr(r0), ptr(nb), N, stride)
        _abi_fwd("table", first, d, 3, h, csr, W, m, rz, c, hout, tab)
        torch.cuda.synchronize()
        out = dict(m=m.clone(), rz_z=rz[:, d:].clone(), c=c.clone(), hout=hout.clone())
        if not first:
            out["rz_r"] = rz[:, :d].clone()
        rz[:N] = nan_dead(rz[:N]); c[:N] = nan_dead(c[:N])           # the backward's inputs: dead rows NaN again
        _abi_bwd("table", first, d, 3, dhout, h, rz, c, csrT, W, dh, gda, rh, tab)
        torch.cuda.synchronize()
        out.update(dh=dh, gda=gda)
        if not first:
            out["rh"] = rh
        res[stride] = out
    for name, x in res[128].items():
        y = res[0][name]
        assert torch.isnan(x[N:]).all() and torch.isnan(y[N:]).all(), name       # the canary behind mt_rows
        x, y = x[:N], y[:N]
        assert (x[~live] == 0).all(), name
        assert torch.isfinite(x[live]).all(), name
        assert torch.equal(x[live], y[live]), name
        assert torch.isnan(y[~live]).all(), name          # (without a stride nothing is written there)
    if first:                                            # no r: its half of rz is not written, the da_r block is zeros
        assert torch.isnan(rz[:N][live][:, :d]).all() and (res[0]["gda"][:N][live][:, 5 * d:6 * d] == 0).all()
    assert res[128]["hout"][:N][live].abs().max() > 0 and res[128]["gda"][:N][live].abs().max() > 0
    # the table entries refuse a stride that is no multiple of 32 or shorter than a full tile, and a missing table
    hout = torch.empty(N, d, device=dev())
    for tab in ((ptr(r0), ptr(nb), N, 96), (ptr(r0), ptr(nb), N, 130), (None, ptr(nb), N, 0), (ptr(r0), None, N, 0), (ptr(r0), ptr(nb), 0, 0)):
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_fwd("table", first, d, 3, h, csr, W, None, None, None, hout, tab)
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_bwd("table", first, d, 3, dhout, h, rz, c, csrT, W, dh, gda, rh, tab)


# ---- encoder level: pairs of the hand-made store, every molecule on both sides and several times ----
I1 = np.array([0, 1, 2, 8, 3, 3, 9, 1, 7, 5, 5, 4, 6]); I2 = np.array([1, 0, 8, 8, 4, 3, 1, 9, 0, 5, 2, 7, 6])
LAB = (np.arange(13).reshape(-1, 1) % 2).astype(np.int32)
ENC = {"dev": "ggnn-dev", "loop": "ggnn-self-loop"}


def _world():
    if "world" not in _CACHE:
        from bmp import packed
        ms = packed.MolStore(_hand_store())
        _CACHE["world"] = (ms, packed.DeviceMolStore(ms, dev()))
    return _CACHE["world"]


def _pair_params(kind, attn, d):
    dr = O._Draw(21, torch.float64, 0.1)
    if attn == "nie":
        O.init_nie(dr, "attn/", d, d, 8)
    O.init_mlp(dr, "mlp/", 2 * d, 1, (32, 16))
    p = dict(dr.p)
    p.update(R.make_params(kind, 60 + len(kind), d, d, LAYERS, False, prefix="graph_conv/"))
    return p


def _pair_model(kind, attn, d=64):
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    model = build_pair_predictor(encoder=ENC[kind], hidden_dim=d, out_dim=d, n_layers=LAYERS, weight_tying=False, attn=attn).to(dev())
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
    ds = _world()[1]
    pb, t = packed.pack_from_store_device(ds, [I1, I2], labels=LAB)
    eb, t2 = enclayout.encode_from_store_device(ds, [I1, I2], labels=LAB, dedup=dedup, n_cu=n_cu)
    assert eb.n_encoded == (10 if dedup else 26)
    nb = eb.pb_enc.mt_nblk.cpu().numpy()
    assert nb.min() >= 1 and nb.max() == 4 and eb.pb_enc.mt_row0 is not None and not eb.pb_enc.oversized
    return pb, t, eb, t2


def _atoms_by_molecule(rows, pb):
    """The real atoms' rows of a row tensor on ``pb``, molecule by molecule in instance order."""
    r0 = pb.mol_row0.cpu().long().tolist()
    return torch.cat([rows[r0[i]:r0[i] + COUNTS[k]] for i, k in enumerate(np.concatenate((I1, I2)))])


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
@pytest.mark.parametrize("kind", ["dev", "loop"])
def test_encoders_train_in_the_encoder_layout(kind, attn, dedup, n_cu, table_on):
    pb, t, eb, t2 = _batches(dedup, n_cu)
    model = _pair_model(kind, attn)
    assert model.training
    inst, took = _took(lambda: _pair_run(model, pb, t))
    assert took == ({"fused": LAYERS, "composed": 0} if kind == "loop" else {"fused": 0, "composed": 0}), took
    at_inst = model.graph_conv.get_atom_array(-1) if kind == "dev" else model.graph_conv.get_atom_array()
    enc, took = _took(lambda: _pair_run(model, eb, t2))
    assert took == ({"fused": LAYERS, "composed": 0} if kind == "loop" else {"fused": 0, "composed": 0}), took
    tag = f"{kind} attn={attn} dedup={dedup} n_cu={n_cu}"
    for k in ("y", "g1", "g2"):
        close(enc[k], inst[k], f"{tag}: {k} vs per-instance", tol=1e-5)
    gmax = max(v.abs().max().item() for v in inst["grads"].values())
    assert sorted(enc["grads"]) == sorted(inst["grads"])
    for name, gr in enc["grads"].items():
        # (1e-3 of the largest gradient as the floor of a parameter's scale: test_gpu_ggate_enc.py)
        close(gr, inst["grads"][name], f"{tag}: grad {name} vs per-instance", tol=1e-5, floor=1e-3 * gmax)
    assert any(v.abs().max() > 0 for k, v in enc["grads"].items() if k.startswith("graph_conv/message_layers"))
    # the atom array handed to the co-attention: the last step's states on the instance rows
    at_enc = model.graph_conv.get_atom_array(-1) if kind == "dev" else model.graph_conv.get_atom_array()
    assert at_enc.pb is eb.pb
    close(_atoms_by_molecule(at_enc.rows, eb.pb), _atoms_by_molecule(at_inst.rows, pb), f"{tag}: last-step atoms", tol=1e-5)
    if kind == "dev":
        assert model.graph_conv.get_atom_array() is at_enc and model.graph_conv.get_atom_array(LAYERS - 1) is at_enc
        for step in (0, 1, -2):
            with pytest.raises(RuntimeError, match="per-instance batch form"):
                model.graph_conv.get_atom_array(step)
        with pytest.raises(RuntimeError, match="per-instance batch form"):
            model.graph_conv.get_g_list()
        model(pb)                                        # a per-instance call brings every step back
        assert len(model.graph_conv.get_g_list()) == LAYERS and model.graph_conv.get_atom_array(0).rows.shape[0] == pb.n_rows


def test_self_loop_paths_follow_the_switch(monkeypatch):
    from bmp import functional as Fn
    pb, t, eb, t2 = _batches(True, 5)
    model = _pair_model("loop", None)
    res = {}
    for on in (True, False):
        monkeypatch.setitem(Fn.LOOP_TABLE_DEFAULT, 64, on)
        res[on], took = _took(lambda: _pair_run(model, eb, t2))
        assert took == ({"fused": LAYERS, "composed": 0} if on else {"fused": 0, "composed": LAYERS}), (on, took)
    for k in ("y", "g1", "g2"):
        close(res[True][k], res[False][k], f"table kernels vs composed: {k}", tol=1e-5)
    gmax = max(v.abs().max().item() for v in res[False]["grads"].values())
    for name, gr in res[True]["grads"].items():
        close(gr, res[False]["grads"][name], f"table kernels vs composed: grad {name}", tol=1e-5, floor=1e-3 * gmax)
    small = _pair_model("loop", None, d=32)              # hidden 32 has no fused self-loop step: composed either way
    for on in (True, False):
        monkeypatch.setitem(Fn.LOOP_TABLE_DEFAULT, 64, on)
        _r, took = _took(lambda: _pair_run(small, eb, t2))
        assert took == {"fused": 0, "composed": LAYERS}, (on, took)
        _r, took = _took(lambda: _pair_run(small, pb, t))
        assert took == {"fused": 0, "composed": LAYERS}, (on, took)


@pytest.mark.parametrize("kind", ["dev", "loop"])
def test_encode_rows_refuses_dropout_in_training_and_concat_hidden(kind):
    from bmp import ggnn_gate
    from bmp.ggnn_dev import DevGGNN, SelfLoopGGNN
    cls = DevGGNN if kind == "dev" else SelfLoopGGNN
    pb, t, eb, t2 = _batches(True, 5)
    enc = cls(out_dim=16, hidden_dim=64, n_layers=2, dropout_rate=0.2).to(dev())
    with pytest.raises(NotImplementedError) as e:
        enc.train().encode_rows(eb.pb_enc)
    assert str(e.value) == "encode_rows: " + ggnn_gate.DROPOUT_LAYOUT_REASON
    h, h0 = enc.eval().encode_rows(eb.pb_enc)            # evaluation mode: dropout is the identity
    assert h.shape == (eb.pb_enc.n_rows, 64) and torch.isfinite(h).all()
    with pytest.raises(NotImplementedError) as e:
        cls(out_dim=16, hidden_dim=64, n_layers=2, concat_hidden=True).to(dev()).eval().encode_rows(eb.pb_enc)
    assert str(e.value) == "encode_rows: " + ggnn_gate.CONCAT_LAYOUT_REASON


# ---- the fixed-shape batch ----
def _static_model():
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.ggnn_dev import SelfLoopGGNN
    torch.manual_seed(5)
    enc = SelfLoopGGNN(out_dim=16, hidden_dim=64, n_layers=3, weight_tying=False)
    return GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev())


def test_static_batch_eager_step_equals_the_packed_step(table_on):
    """Batch k0 holds the store's tallest molecules and batch k1, loaded into the same arrays afterwards, its shortest: rows that
    k0 left behind in a dead block would enter k1's weight gradients."""
    Fn = table_on
    from bmp import packed
    from bmp.dp import FlatAdam
    ds, by_size, sizes = _static_world()
    B = 8
    model = _static_model()
    opt = FlatAdam(model, alpha=1e-3)
    sb = packed.StaticPairBatch(ds, B)
    rs = np.random.RandomState(4)
    tall, short = by_size[:2 * B], by_size[-2 * B:]
    assert min(sizes[k] for k in tall) > 64 and max(sizes[k] for k in short) < 31        # 3-4 live blocks, then one
    for tag, sel in (("k0 tallest", tall), ("k1 shortest", short)):
        i1, i2 = sel[:B], sel[B:]
        lab = rs.randint(0, 2, (B, 1)).astype(np.int32)
        pb, t = packed.pack_from_store_device(ds, [i1, i2], labels=lab)
        sb.load([i1, i2], lab); sb.reset_derived(); sb.emit()
        assert sb.pb.mt_row0 is not None and sb.pb.tile_stride == 128
        (loss, took) = _took(lambda: opt.functional_loss(pb, t=t))
        assert took == {"fused": 3, "composed": 0}, took
        loss.backward(); opt.collect_grads()
        y_ref, g_ref, l_ref = model.y.detach().clone(), opt.grad.clone(), loss.detach().clone()
        (loss, took) = _took(lambda: opt.functional_loss(sb.pb, t=sb.t))
        assert took == {"fused": 3, "composed": 0}, took
        loss.backward(); opt.collect_grads()
        close(model.y.detach(), y_ref, f"static self loop {tag}: logits", tol=1e-5)
        close(loss.detach().reshape(1), l_ref.reshape(1), f"static self loop {tag}: loss", tol=1e-5)
        close(opt.grad, g_ref, f"static self loop {tag}: flat gradient", tol=1e-5)


def test_fit_runs_a_self_loop_model_in_every_layout(table_on):
    """``fit`` over PairBatches per instance, in the encoder layout with dedup and as replays of one recorded step
    (layout="static"; the short last batch of a pass runs launch by launch): the same losses epoch by epoch, at the bound of
    tests/test_trainer.py's layout comparison (different summation orders only)."""
    Fn = table_on
    from bmp import packed, synth, trainer as Tr
    from bmp.dp import FlatAdam
    from bmp.predictor import build_pair_predictor
    store = synth.make_store(40, seed=3, n_lo=4, n_hi=40, n_mean=16)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev())
    rs = np.random.RandomState(1)
    i1, i2 = rs.randint(0, 40, 200), rs.randint(0, 40, 200)
    nat = np.array([m.n for m in store])
    lab = ((nat[i1] + nat[i2]) % 2).astype(np.int32).reshape(-1, 1)
    runs, took = {}, {}
    for name, kw in (("instance", {}), ("dedup", dict(layout="encoder", dedup=True)), ("static", dict(layout="static"))):
        torch.manual_seed(0)
        model = build_pair_predictor(encoder="ggnn-self-loop", hidden_dim=64, out_dim=32, n_layers=2, attn="nie", head=4).to(dev())
        opt = FlatAdam(model, alpha=2e-3)
        tr = Tr.PairBatches(ds, i1[:144], i2[:144], lab[:144], 32, shuffle=True, seed=2, **kw)
        va = Tr.PairBatches(ds, i1[144:], i2[144:], lab[144:], 32, **kw)
        assert len(tr) == 5 and len(va) == 2
        tr.check_encoder(model)
        runs[name], took[name] = _took(lambda: Tr.fit(model, opt, tr, va, epochs=2))
    assert took["dedup"]["composed"] == 0 and took["dedup"]["fused"] > 0, took          # the table kernels, every step
    assert took["static"]["composed"] == 0 and 0 < took["static"]["fused"] < took["instance"]["fused"], took       # replays
    for name in ("dedup", "static"):
        for a, b in zip(runs["instance"], runs[name]):
            for key in ("main/loss", "validation/main/loss"):
                assert abs(a[key] - b[key]) <= 2e-4 * abs(a[key]), (name, key, a[key], b[key])


def test_static_batch_recorded_step_replays_on_the_table_kernels(table_on):
    Fn = table_on
    from bmp import packed
    from bmp.dp import FlatAdam, GraphedTrainStep
    ds, by_size, _sizes = _static_world()
    B, steps = 8, 4
    eager, graphed = _static_model(), _static_model()
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
        mark = dict(Fn.LOOP_PATHS)
        lg.append(float(stepper(sb).detach()))
        assert Fn.LOOP_PATHS["composed"] == mark["composed"]          # the recording took the table kernels, every call of it
        assert (Fn.LOOP_PATHS["fused"] > mark["fused"]) == (k == 0)   # ... and a replay runs no Python step
    assert len(stepper.graphs) == 1 and og.t == oe.t == steps
    close(torch.tensor(lg), torch.tensor(le), f"recorded self-loop step: losses of {steps} steps", tol=1e-4)
    close(og.flat, oe.flat, f"recorded self-loop step: parameters after {steps} steps", tol=1e-4)
    assert not np.allclose(le[0], le[-1])
