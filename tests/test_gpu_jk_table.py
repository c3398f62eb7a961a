"""The jumping-knowledge step on a TILE TABLE (csrc/bmp_jk_table.hip), the 'mean' aggregator on a row count and the encoders of
bmp/ggnn_jk.py in the encoder layout, under de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (tests/jk_ref.py), 1e-5 between two
float32 forms of the same step, 1e-4 for parameters after several replayed steps (test_gpu_static_batch.py).  The store and the
three tables are tests/test_gpu_ggate_enc.py's (their properties: tests/test_ggdev_enc_build.py), the pairs, the stride case and
the batch helpers tests/test_gpu_ggdev_enc.py's; every case is under 800 rows at d = 64, one repeats at d = 128.  The tests that
go through ``jk_step`` force ``JK_TABLE_DEFAULT`` on: they do not depend on the measured default."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jk_ref as R                                     # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from parity_util import close                          # noqa: E402
from test_gpu_ops import dev, to_dev                   # noqa: E402
from test_gpu_ggate_enc import _dense_adj, _static_world, _table                          # noqa: E402
from test_gpu_ggdev_enc import I1, I2, LAYERS, _atoms_by_molecule, _batches, _pair_run, _stride_case      # noqa: E402

NAMES = ("h", "WT", "bE", "WsT", "bs", "AU", "bU")
GRADS = ("dh", "dWT", "dbE", "dWsT", "dbs", "dAU", "dbU")
KINDS = ((1, False), (2, True), (2, False))            # (ng, self loop): jknet, jk_gru with and without its self loop
_CACHE = {}


@pytest.fixture
def table_on(monkeypatch):
    from bmp import functional as Fn
    for key in Fn.JK_TABLE_DEFAULT:
        monkeypatch.setitem(Fn.JK_TABLE_DEFAULT, key, True)
        monkeypatch.setitem(Fn.JK_STEP_DEFAULT, key, True)
    return Fn


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.JK_PATHS)
    out = fn()
    return out, {k: Fn.JK_PATHS[k] - before[k] for k in before}


# ---- one step on the three tables ----
# (table, d, ng, loop): the generator seed of the case's operands, the first >= 400 at which the restatement alone meets the relu
# kink condition  min |pre64| >= KINK_FACTOR * max |pre32 - pre64|  over all N * ng * d pre-activations with half as much again
# to spare (a margin of 12: a float32 restatement that sums in another order still passes the asserted 8).  ``_kink`` below
# computes both sides, ``_search_seeds`` is the search; both run on the CPU.  Beside each: the margin min |pre64| / max |pre32 - pre64|.
SEEDS = {
    ("own", 64, 1, False): 400,  # 47 x
    ("own", 64, 2, True): 416,  # 30 x
    ("own", 64, 2, False): 406,  # 27 x
    ("shared", 64, 1, False): 400,  # 27 x
    ("shared", 64, 2, True): 400,  # 23 x
    ("shared", 64, 2, False): 401,  # 15 x
    ("seven", 64, 1, False): 400,  # 76 x
    ("seven", 64, 2, True): 400,  # 71 x
    ("seven", 64, 2, False): 400,  # 18 x
    ("own", 128, 1, False): 402,  # 12 x
    ("own", 128, 2, True): 487,  # 14 x
    ("own", 128, 2, False): 582,  # 14 x
}
SEED_MARGIN = 1.5                                      # the search's: KINK_FACTOR * SEED_MARGIN


def _operands(name, d, ng, loop, seed=None):
    """Float64 operands of one step on table ``name`` in the kernel's layouts, drawn once, and the cotangent."""
    key = ("ops", name, d, ng, loop, seed)
    if key not in _CACHE:
        N = _table(name).pb_enc.n_rows
        g = torch.Generator().manual_seed(SEEDS[(name, d, ng, loop)] if seed is None else seed)
        r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
        nu = ng * d
        o = dict(h=r(N, d), WT=0.5 * r(4 * d, d) / d ** 0.5, bE=0.3 * r(4, d), WsT=0.5 * r(d, d) / d ** 0.5, bs=0.3 * r(d),
                 AU=r(2 * d, nu) / (2 * d) ** 0.5, bU=0.3 * r(nu), c=r(N, nu))
        if not loop:
            o["WsT"] = o["bs"] = None
        _CACHE[key] = o
    return _CACHE[key]


def _ref_params(q, d, ng, loop):
    """The operands as tests/jk_ref.py's parameters, the table's rows one dense 'molecule' whose atom ids are its row numbers."""
    z = lambda *s: torch.zeros(*s, dtype=q["h"].dtype)
    p = {"embed/W": q["h"],
         "message_layers/0/W": q["WT"].view(4, d, d).permute(2, 0, 1).reshape(4 * d, d),       # feature 4 c + e <- WT[e d + k, c]
         "message_layers/0/b": q["bE"].t().reshape(4 * d),
         ("update_layer/0" if ng == 1 else "update_layers_0/0") + "/W": q["AU"].t(),
         ("update_layer/0" if ng == 1 else "update_layers_0/0") + "/b": q["bU"],
         "i_layers/0/W": z(4, 2 * d), "i_layers/0/b": z(4), "j_layers/0/W": z(4, d), "j_layers/0/b": z(4)}
    if ng == 2:
        for n, k_in in (("W_r", 2 * d), ("W_z", 2 * d), ("W", 2 * d), ("U_r", d), ("U_z", d), ("U", d)):
            p[f"update_layer/{n}/W"], p[f"update_layer/{n}/b"] = z(d, k_in), z(d)
    if loop:
        p["self_loop_layer/W"], p["self_loop_layer/b"] = q["WsT"].t(), q["bs"]
    return p


def _ref_step(o, adj, d, ng, loop, dtype, backward=True):
    """tests/jk_ref.py's step -- the loop body of its ``forward``, op for op: the message, jk_gru's self loop, relu(update [h, m])
    -- on the table's rows as one dense molecule of N positions; the leaves are the kernel-layout operands, so their gradients
    come out in the kernel's layouts.  The pre-activations are checked against what ``jk_ref.forward`` itself hands out.
    (out, pre, {operand: gradient})."""
    q = {k: (None if o[k] is None else o[k].to(dtype).clone().requires_grad_(backward)) for k in NAMES}
    p = _ref_params(q, d, ng, loop)
    N = o["h"].shape[0]
    h = q["h"][None]
    m = O.ggnn_message(h, torch.as_tensor(adj).to(dtype), p["message_layers/0/W"], p["message_layers/0/b"])
    if loop:
        m = m + O.linear(h, p["self_loop_layer/W"], p["self_loop_layer/b"])
    a = O.linear(torch.cat((h[0], m[0]), dim=1), q["AU"].t(), q["bU"])
    out = torch.relu(a)
    pre = []
    with torch.no_grad():
        R.forward("jknet" if ng == 1 else "jk_gru", p, np.arange(N)[None], adj, 1, self_loop=loop, aggr="concat", pre=pre)
    assert len(pre) == 1 and torch.equal(pre[0], a.detach())
    if not backward:
        return out.detach(), a.detach(), None
    (out * o["c"].to(dtype)).sum().backward()
    return out.detach(), a.detach(), {k: (None if q[k] is None else q[k].grad) for k in NAMES}


def _kink(name, d, ng, loop, seed=None):
    """(min |pre64|, max |pre32 - pre64|) of the case's float64 and float32 restatements."""
    o = _operands(name, d, ng, loop, seed)
    adj = _dense_adj(_table(name).pb_enc)
    a64 = _ref_step(o, adj, d, ng, loop, torch.float64, backward=False)[1]
    a32 = _ref_step(o, adj, d, ng, loop, torch.float32, backward=False)[1]
    return a64.abs().min().item(), (a32.double() - a64).abs().max().item()


def _search_seeds(start=400):
    """Prints the SEEDS table (CPU only)."""
    for name, d in (("own", 64), ("shared", 64), ("seven", 64), ("own", 128)):
        for ng, loop in KINDS:
            for seed in range(start, start + 4000):
                lo, err = _kink(name, d, ng, loop, seed)
                _CACHE.pop(("ops", name, d, ng, loop, seed))
                if lo >= SEED_MARGIN * R.KINK_FACTOR * err:
                    print(f'    ("{name}", {d}, {ng}, {loop}): {seed},  # {lo / err:.0f} x', flush=True)
                    break


def _restatement(name, d, ng, loop):
    key = ("ref", name, d, ng, loop)
    if key not in _CACHE:
        out, _pre, grads = _ref_step(_operands(name, d, ng, loop), _dense_adj(_table(name).pb_enc), d, ng, loop, torch.float64)
        _CACHE[key] = (out, grads)
    return _CACHE[key]


def _args(o, grad):
    f = lambda x: None if x is None else x.float().to(dev()).requires_grad_(grad)
    return {k: f(o[k]) for k in NAMES}


def _run_step(name, d, ng, loop, pb, fused):
    """One step forward and backward in float32 on the device: (out, {operand: gradient})."""
    from bmp import functional as Fn
    o = _operands(name, d, ng, loop)
    q = _args(o, True)
    if fused:
        out = Fn.JKStepFn.apply(*(q[k] for k in NAMES), pb)
    else:
        out = Fn.jk_step(*(q[k] for k in NAMES), pb, fused=False)
    (out * o["c"].float().to(dev())).sum().backward()
    return out.detach(), {k: (None if q[k] is None else q[k].grad) for k in NAMES}


def _compare(a, b, tag, tol):
    close(a[0], b[0], f"{tag}: out", tol=tol)
    for k, nm in zip(NAMES, GRADS):
        if b[1][k] is not None:
            close(a[1][k], b[1][k], f"{tag}: {nm}", tol=tol)


@pytest.mark.parametrize("ng,loop", KINDS)
@pytest.mark.parametrize("name,d", [("own", 64), ("shared", 64), ("seven", 64), ("own", 128)])
def test_table_step_against_composed_and_restatement(name, d, ng, loop, table_on):
    Fn = table_on
    pb = to_dev(_table(name).pb_enc)
    r0, nb = pb.mt_row0.cpu().numpy(), pb.mt_nblk.cpu().numpy()
    cover = np.zeros(pb.n_rows, dtype=int)
    for a, k in zip(r0, nb):
        cover[a:a + 32 * k] += 1
    assert (cover == 1).all() and pb.n_rows < 800        # the table's tiles abut and hold every row once
    lo, err = _kink(name, d, ng, loop)
    print(f"[kink] {name} d={d} ng={ng} loop={loop}: min |pre64| {lo:.3e}, max |pre32 - pre64| {err:.3e}, margin {lo / err:.1f} x")
    assert lo >= R.KINK_FACTOR * err, (lo, err)          # no relu of the case sits on its kink at float32 precision
    ref = _restatement(name, d, ng, loop)
    fused, took = _took(lambda: _run_step(name, d, ng, loop, pb, True))
    assert took == {"fused": 1, "composed": 0}, took
    comp, took = _took(lambda: _run_step(name, d, ng, loop, pb, False))
    assert took == {"fused": 0, "composed": 1}, took
    tag = f"{name} d={d} ng={ng} loop={loop}"
    _compare(fused, comp, f"table {tag} vs composed", 1e-5)
    _compare(fused, ref, f"table {tag} vs float64", 1e-4)
    _compare(comp, ref, f"composed {tag} vs float64", 1e-4)
    again = _run_step(name, d, ng, loop, pb, True)
    assert torch.equal(again[0], fused[0])
    assert all(torch.equal(again[1][k], fused[1][k]) for k in NAMES if fused[1][k] is not None)
    with torch.no_grad():                                # forward-only evaluation: null m
        args = list(_args(_operands(name, d, ng, loop), False).values())
        o0, took = _took(lambda: Fn.JKStepFn.apply(*args, pb))
        assert took == {"fused": 1, "composed": 0} and torch.equal(o0, fused[0])
        o1, took = _took(lambda: Fn.jk_step(*args, pb))                   # ... and what jk_step picks with the switch on
        assert took == {"fused": 1, "composed": 0} and torch.equal(o1, fused[0])


# ---- through the C ABI ----
def _weights(d, ng, loop, seed):
    from bmp.functional import pack_k4
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    WT, WsT, AU = 0.5 * rnd(4 * d, d) / d ** 0.5, 0.5 * rnd(d, d) / d ** 0.5, rnd(2 * d, ng * d) / (2 * d) ** 0.5
    W = dict(WTp=pack_k4(WT), bE=0.3 * rnd(4, d), WsTp=pack_k4(WsT), bs=0.3 * rnd(d), AUp=pack_k4(AU), bU=0.3 * rnd(ng * d),
             Wnp=pack_k4(WT.t()), Wsp=pack_k4(WsT.t()), Unp=pack_k4(AU.t()))
    if not loop:
        W["WsTp"] = W["bs"] = W["Wsp"] = None
    return W


def _abi_fwd(entry, ng, d, n_tiles, h, csr, W, m, out, tab=()):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    name = f"bmp_jk_step_{entry}_fwd"
    check(getattr(_lib.lib(), name)(ng, ptr(h), n_tiles, d, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ptr(W["WTp"]), ptr(W["bE"]),
                                    ptr(W["WsTp"]), ptr(W["bs"]), ptr(W["AUp"]), ptr(W["bU"]), ptr(m), ptr(out), *tab, stream()), name)


def _abi_bwd(entry, ng, d, n_tiles, dout, out, csrT, W, dh, gda, tab=()):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    name = f"bmp_jk_step_{entry}_bwd"
    check(getattr(_lib.lib(), name)(ng, ptr(dout), ptr(out), n_tiles, d, ptr(csrT[0]), ptr(csrT[1]), ptr(csrT[2]), ptr(W["Wnp"]),
                                    ptr(W["Wsp"]), ptr(W["Unp"]), ptr(dh), ptr(gda), *tab, stream()), name)


@pytest.mark.parametrize("ng,loop", KINDS)
@pytest.mark.parametrize("d", [64, 128])
def test_table_of_whole_tiles_is_the_whole_tile_kernel_bit_for_bit(d, ng, loop):
    """Every table entry a four-block tile at 128 t, on the whole-tile batch of tests/jk_ref.py's "fixture" (three tiles, all four
    bond types): the products run in the same order, so every written array is bit-identical."""
    from bmp._lib import ptr
    pb = to_dev(R.data("fixture")["pb"])
    assert pb.mt_row0 is None and not pb.oversized and pb.n_tiles >= 3
    N, nt = pb.n_rows, pb.n_tiles
    csr, csrT = (pb.csr_ptr, pb.csr_col, pb.csr_val), (pb.csrT_ptr, pb.csrT_col, pb.csrT_val)
    W = _weights(d, ng, loop, 40 + d)
    g = torch.Generator().manual_seed(41)
    h, dout = torch.randn(N, d, generator=g).to(dev()), torch.randn(N, ng * d, generator=g).to(dev())
    r0 = torch.arange(nt, dtype=torch.int32, device=dev()) * 128
    nb = torch.full((nt,), 4, dtype=torch.int32, device=dev())
    res = {}
    for entry, tab in (("tile", ()), ("table", (ptr(r0), ptr(nb), N, 0))):
        z = lambda n: torch.zeros(N, n, device=dev())
        m, out, dh, gda = z(d), z(ng * d), z(d), z((5 if loop else 4) * d + ng * d)
        _abi_fwd(entry, ng, d, nt, h, csr, W, m, out, tab)
        _abi_bwd(entry, ng, d, nt, dout, out, csrT, W, dh, gda, tab)
        torch.cuda.synchronize()
        res[entry] = dict(m=m, out=out, dh=dh, gda=gda)
    for k, x in res["table"].items():
        assert torch.isfinite(x).all(), k
        print(f"[whole tiles] d={d} ng={ng} loop={loop} {k}: max |table - tile| = {(x - res['tile'][k]).abs().max().item():.3e}")
        assert torch.equal(x, res["tile"][k]), (k, (x - res["tile"][k]).abs().max().item())
    assert res["table"]["out"].abs().max() > 0 and res["table"]["gda"].abs().max() > 0


@pytest.mark.parametrize("ng,loop", KINDS)
def test_fixed_stride_clears_the_dead_rows(ng, loop):
    """Through the C ABI at d = 64 on tiles of 1, 3 and 4 live blocks at stride 128: every output prefilled with NaN, the dead
    rows of h, dout and (for the backward) out NaN too (never read), and a 128-row NaN canary behind mt_rows in every written
    array.  With tile_stride = 128 the rows of the dead blocks are exactly 0 in m, out, dh and gda and no NaN is left anywhere;
    the live rows equal the dense-row run (tile_stride = 0, which leaves the dead rows alone) of the same molecules; the canary
    stays NaN either way."""
    from bmp._lib import ptr
    d, N, C = 64, 384, 128
    csr, csrT, r0, nb, live = _stride_case()
    W = _weights(d, ng, loop, 77)
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    nan_dead = lambda x: torch.where(live[:, None], x, torch.full_like(x, float("nan")))
    h, dout = nan_dead(rnd(N, d)), nan_dead(rnd(N, ng * d))
    res = {}
    for stride in (128, 0):
        nan = lambda n: torch.full((N + C, n), float("nan"), device=dev())
        m, out, dh, gda = nan(d), nan(ng * d), nan(d), nan((5 if loop else 4) * d + ng * d)
        tab = (ptr(r0), ptr(nb), N, stride)
        _abi_fwd("table", ng, d, 3, h, csr, W, m, out, tab)
        torch.cuda.synchronize()
        res[stride] = dict(m=m.clone(), out=out.clone())
        out[:N] = nan_dead(out[:N])                      # the backward's input: dead rows NaN again
        _abi_bwd("table", ng, d, 3, dout, out, csrT, W, dh, gda, tab)
        torch.cuda.synchronize()
        res[stride].update(dh=dh, gda=gda)
    for name, x in res[128].items():
        y = res[0][name]
        assert torch.isnan(x[N:]).all() and torch.isnan(y[N:]).all(), name       # the canary behind mt_rows
        x, y = x[:N], y[:N]
        assert not torch.isnan(x).any(), name
        assert (x[~live] == 0).all(), name
        assert torch.isfinite(x[live]).all(), name
        close(x[live], y[live], f"fixed stride ng={ng} loop={loop}: live rows of {name} vs dense rows", tol=1e-5)
        assert torch.isnan(y[~live]).all(), name          # (without a stride nothing is written there)
    assert res[128]["out"][:N][live].abs().max() > 0 and res[128]["gda"][:N][live].abs().max() > 0
    # the table entries refuse a stride that is no multiple of 32 or shorter than a full tile, and a missing table
    out = torch.empty(N, ng * d, device=dev())
    for tab in ((ptr(r0), ptr(nb), N, 96), (ptr(r0), ptr(nb), N, 130), (None, ptr(nb), N, 0), (ptr(r0), None, N, 0), (ptr(r0), ptr(nb), 0, 0)):
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_fwd("table", ng, d, 3, h, csr, W, None, out, tab)
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_bwd("table", ng, d, 3, dout, out, csrT, W, dh, gda, tab)


# ---- 'mean' on a row count ----
@pytest.mark.parametrize("T_", [1, 3, 8])
@pytest.mark.parametrize("n_rows", [32, 96, 160])
def test_mean_on_a_row_count(n_rows, T_):
    """bmp_jk_mean_fwd / _bwd against the torch expression at 1e-6 of the max-abs (a sum of at most eight products), in buffers
    one row longer than n_rows whose last row stays what it was."""
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    L, d = _lib.lib(), 64
    g = torch.Generator().manual_seed(100 * n_rows + T_)
    hs = [torch.randn(n_rows + 1, d, generator=g).to(dev()) for _ in range(T_)]
    dy = torch.randn(n_rows + 1, d, generator=g).to(dev())
    y = torch.full((n_rows + 1, d), 7.0, device=dev())
    dhs = [torch.full((n_rows + 1, d), 7.0, device=dev()) for _ in range(T_)]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    check(L.bmp_jk_mean_fwd(arr(hs), T_, n_rows, d, ptr(y), stream()), "bmp_jk_mean_fwd")
    check(L.bmp_jk_mean_bwd(ptr(dy), T_, n_rows, d, arr(dhs), stream()), "bmp_jk_mean_bwd")
    torch.cuda.synchronize()
    want = torch.stack([x[:n_rows].double() for x in hs]).mean(dim=0)
    close(y[:n_rows], want, f"mean n_rows={n_rows} T={T_}: y", tol=1e-6)
    assert (y[n_rows] == 7.0).all()
    for t, x in enumerate(dhs):
        close(x[:n_rows], dy[:n_rows].double() / T_, f"mean n_rows={n_rows} T={T_}: dh[{t}]", tol=1e-6)
        assert (x[n_rows] == 7.0).all()


# ---- encoder level: pairs of the hand-made store, every molecule on both sides and several times ----
KIND = {"jknet-max": ("jknet", "max", False), "jknet-mean": ("jknet", "mean", False), "jk-gru": ("jk_gru", None, False),
        "jk-gru+self_loop": ("jk_gru", None, True)}


def _pair_params(kind, attn, d):
    ref_kind, _aggr, loop = KIND[kind]
    dr = O._Draw(21, torch.float64, 0.1)
    if attn == "nie":
        O.init_nie(dr, "attn/", d, d, 8)
    O.init_mlp(dr, "mlp/", 2 * d, 1, (32, 16))
    p = dict(dr.p)
    # (the pair predictor builds jknet with its one tied update layer, jk_gru with one per untied message layer)
    p.update(R.make_params(ref_kind, 60 + len(kind), d, d, LAYERS, False, ref_kind == "jknet", self_loop=loop, prefix="graph_conv/"))
    return p


def _pair_model(kind, attn, d=64):
    from bmp.ggnn_jk import JKGruGGNN
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    ref_kind, aggr, loop = KIND[kind]
    model = build_pair_predictor(encoder="ggnn-jknet" if ref_kind == "jknet" else "ggnn-jk-gru", hidden_dim=d, out_dim=d,
                                 n_layers=LAYERS, weight_tying=False, attn=attn, layer_aggr=aggr or "attn")
    if loop:
        model.graph_conv = JKGruGGNN(out_dim=d, hidden_dim=d, n_layers=LAYERS, weight_tying=False, update_tying=False, self_loop=True)
    model = model.to(dev())
    load_param_dict(model, _pair_params(kind, attn, d))
    return model


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
@pytest.mark.parametrize("kind", list(KIND))
def test_encoders_train_in_the_encoder_layout(kind, attn, dedup, n_cu, table_on):
    pb, t, eb, t2 = _batches(dedup, n_cu)
    model = _pair_model(kind, attn)
    assert model.training and model.graph_conv.rows_reason() is None
    inst, took = _took(lambda: _pair_run(model, pb, t))
    assert took == {"fused": LAYERS, "composed": 0}, took
    at_inst = model.graph_conv.get_atom_array()
    enc, took = _took(lambda: _pair_run(model, eb, t2))
    assert took == {"fused": LAYERS, "composed": 0}, took
    tag = f"{kind} attn={attn} dedup={dedup} n_cu={n_cu}"
    for k in ("y", "g1", "g2"):
        close(enc[k], inst[k], f"{tag}: {k} vs per-instance", tol=1e-5)
    loss_i, loss_e = model.loss(inst["y"], t).detach().reshape(1), model.loss(enc["y"], t2).detach().reshape(1)
    close(loss_e, loss_i, f"{tag}: loss vs per-instance", tol=1e-5)
    gmax = max(v.abs().max().item() for v in inst["grads"].values())
    assert sorted(enc["grads"]) == sorted(inst["grads"])
    for name, gr in enc["grads"].items():
        # (1e-3 of the largest gradient as the floor of a parameter's scale: test_gpu_ggate_enc.py)
        close(gr, inst["grads"][name], f"{tag}: grad {name} vs per-instance", tol=1e-5, floor=1e-3 * gmax)
    assert any(v.abs().max() > 0 for k, v in enc["grads"].items() if k.startswith("graph_conv/message_layers"))
    # the atom array handed to the co-attention: what the readout read (jknet: the aggregate) on the instance rows
    at_enc = model.graph_conv.get_atom_array()
    assert at_enc.pb is eb.pb
    close(_atoms_by_molecule(at_enc.rows, eb.pb), _atoms_by_molecule(at_inst.rows, pb), f"{tag}: atoms", tol=1e-5)


def test_paths_follow_the_switch(monkeypatch):
    from bmp import functional as Fn
    pb, t, eb, t2 = _batches(True, 5)
    model = _pair_model("jk-gru", None)
    res = {}
    for on in (True, False):
        monkeypatch.setitem(Fn.JK_TABLE_DEFAULT, ("jk_gru", 64), on)
        res[on], took = _took(lambda: _pair_run(model, eb, t2))
        assert took == ({"fused": LAYERS, "composed": 0} if on else {"fused": 0, "composed": LAYERS}), (on, took)
    for k in ("y", "g1", "g2"):
        close(res[True][k], res[False][k], f"table kernels vs composed: {k}", tol=1e-5)
    gmax = max(v.abs().max().item() for v in res[False]["grads"].values())
    for name, gr in res[True]["grads"].items():
        close(gr, res[False]["grads"][name], f"table kernels vs composed: grad {name}", tol=1e-5, floor=1e-3 * gmax)


def test_encode_rows_refuses_concat_hidden_training_dropout_and_attn():
    from bmp import ggnn_gate
    from bmp.ggnn_jk import JK_ATTN_LAYOUT_REASON, JKGruGGNN, JKNetGGNN
    pb, t, eb, t2 = _batches(True, 5)
    for make in (lambda **kw: JKNetGGNN(out_dim=16, hidden_dim=64, n_layers=2, layer_aggr="mean", **kw),
                 lambda **kw: JKGruGGNN(out_dim=16, hidden_dim=64, n_layers=2, self_loop=True, **kw)):
        enc = make(dropout_rate=0.25).to(dev())
        with pytest.raises(NotImplementedError) as e:
            enc.train().encode_rows(eb.pb_enc)
        assert str(e.value) == "encode_rows: " + ggnn_gate.DROPOUT_LAYOUT_REASON
        before = set(vars(enc))
        y, h0 = enc.eval().encode_rows(eb.pb_enc)        # evaluation mode: dropout is the identity
        assert y.shape == h0.shape == (eb.pb_enc.n_rows, 64) and torch.isfinite(y).all()
        assert set(vars(enc)) == before and enc.atoms is None     # nothing set that the per-instance call would not set
        with pytest.raises(NotImplementedError) as e:
            make(concat_hidden=True).to(dev()).eval().encode_rows(eb.pb_enc)
        assert str(e.value) == "encode_rows: " + ggnn_gate.CONCAT_LAYOUT_REASON
    with pytest.raises(NotImplementedError) as e:
        JKNetGGNN(out_dim=16, hidden_dim=64, n_layers=2, layer_aggr="attn").to(dev()).eval().encode_rows(eb.pb_enc)
    assert str(e.value) == "encode_rows: " + JK_ATTN_LAYOUT_REASON
    one = JKNetGGNN(out_dim=16, hidden_dim=64, n_layers=1, layer_aggr="concat").to(dev()).eval()
    y, h0 = one.encode_rows(eb.pb_enc)                   # 'concat' of one layer: the single step's output
    assert y.shape == (eb.pb_enc.n_rows, 64) and (y >= 0).all() and y.abs().max() > 0


# ---- the fixed-shape batch ----
def _static_model(kind="jk-gru+self_loop"):
    from bmp.ggnn_jk import JKGruGGNN, JKNetGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    torch.manual_seed(5)
    if kind == "jknet-mean":
        enc = JKNetGGNN(out_dim=16, hidden_dim=64, n_layers=3, weight_tying=False, update_tying=False, layer_aggr="mean")
    else:
        enc = JKGruGGNN(out_dim=16, hidden_dim=64, n_layers=3, weight_tying=False, update_tying=False, self_loop=True)
    return GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev())


@pytest.mark.parametrize("kind", ["jk-gru+self_loop", "jknet-mean"])
def test_static_batch_eager_step_equals_the_packed_step(kind, table_on):
    """Batch k0 holds the store's tallest molecules and batch k1, loaded into the same arrays afterwards, its shortest: rows that
    k0 left behind in a dead block would enter k1's weight gradients."""
    from bmp import packed
    from bmp.dp import FlatAdam
    ds, by_size, sizes = _static_world()
    B = 8
    model = _static_model(kind)
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
        close(model.y.detach(), y_ref, f"static {kind} {tag}: logits", tol=1e-5)
        close(loss.detach().reshape(1), l_ref.reshape(1), f"static {kind} {tag}: loss", tol=1e-5)
        close(opt.grad, g_ref, f"static {kind} {tag}: flat gradient", tol=1e-5)


def test_fit_runs_a_jk_gru_model_in_every_layout(table_on):
    """``fit`` over PairBatches per instance, in the encoder layout with dedup and as replays of one recorded step
    (layout="static"; the short last batch of a pass runs launch by launch): the same parameters after two passes."""
    from bmp import packed, synth, trainer as Tr
    from bmp.dp import FlatAdam
    from bmp.predictor import build_pair_predictor
    store = synth.make_store(40, seed=3, n_lo=4, n_hi=40, n_mean=16)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev())
    rs = np.random.RandomState(1)
    i1, i2 = rs.randint(0, 40, 200), rs.randint(0, 40, 200)
    nat = np.array([m.n for m in store])
    lab = ((nat[i1] + nat[i2]) % 2).astype(np.int32).reshape(-1, 1)
    runs, took, flat = {}, {}, {}
    for name, kw in (("instance", {}), ("dedup", dict(layout="encoder", dedup=True)), ("static", dict(layout="static"))):
        torch.manual_seed(0)
        model = build_pair_predictor(encoder="ggnn-jk-gru", hidden_dim=64, out_dim=32, n_layers=2, attn="nie", head=4).to(dev())
        opt = FlatAdam(model, alpha=2e-3)
        tr = Tr.PairBatches(ds, i1[:144], i2[:144], lab[:144], 32, shuffle=True, seed=2, **kw)
        va = Tr.PairBatches(ds, i1[144:], i2[144:], lab[144:], 32, **kw)
        assert len(tr) == 5 and len(va) == 2
        tr.check_encoder(model)
        runs[name], took[name] = _took(lambda: Tr.fit(model, opt, tr, va, epochs=2))
        flat[name] = opt.flat.detach().clone()
    assert took["dedup"]["composed"] == 0 and took["dedup"]["fused"] > 0, took          # the table kernels, every step
    assert took["static"]["composed"] == 0 and 0 < took["static"]["fused"] < took["instance"]["fused"], took       # replays
    for name in ("dedup", "static"):
        for a, b in zip(runs["instance"], runs[name]):
            for key in ("main/loss", "validation/main/loss"):
                print(f"[fit] {name} {key}: {b[key]:.7f} vs per-instance {a[key]:.7f}")
        close(flat[name], flat["instance"], f"fit jk_gru {name}: parameters after two passes vs per-instance", tol=1e-4)


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
        mark = dict(Fn.JK_PATHS)
        lg.append(float(stepper(sb).detach()))
        assert Fn.JK_PATHS["composed"] == mark["composed"]            # the recording took the table kernels, every call of it
        assert (Fn.JK_PATHS["fused"] > mark["fused"]) == (k == 0)     # ... and a replay runs no Python step
    assert len(stepper.graphs) == 1 and og.t == oe.t == steps
    close(torch.tensor(lg), torch.tensor(le), f"recorded jk_gru step: losses of {steps} steps", tol=1e-4)
    close(og.flat, oe.flat, f"recorded jk_gru step: parameters after {steps} steps", tol=1e-4)
    assert not np.allclose(le[0], le[-1])
