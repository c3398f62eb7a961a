"""The NFP layer and readout on a TILE TABLE (csrc/bmp_nfp_table.hip) and the NFP encoder (bmp/nfp.py) in the encoder layout,
under de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (below, in the form of
tests/nfp_ref.py's packed one), 1e-5 between two float32 forms of the same step, 1e-4 for parameters after several replayed
steps, 1e-3 of the largest gradient as a parameter's floor.  The tables' molecules are tests/nfp_tables.py's (every degree class in
every table, the tile tables of tests/enc_tables.py); the stride case, the dense four-block tile and the shared bodies are
tests/table_harness.py's; every case is under 800 rows at d = 64 but the harness's own 13-pair world without dedup, the one-step
cases repeat at d = 128.  The tests that go through the modules force ``NFP_TABLE_DEFAULT`` on: they do not depend on the measured
default."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nfp_ref as NR                                   # noqa: E402
import nfp_tables as NT                                # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from parity_util import close                          # noqa: E402
from test_gpu_ops import dev, to_dev                   # noqa: E402
import table_harness as H                              # noqa: E402

LAYERS = 3
P_PAD = 3.0                                            # the multiplicity of the stride case's pad rows
_CACHE = {}


def _paths():
    from bmp import functional as Fn
    return Fn.NFP_LAYER_PATHS


class _ReadoutPaths:
    """NFP_PATHS' two readout counters under the names of the table families' counters."""
    KEYS = {"fused": "readout_tile", "composed": "readout_rows"}

    def keys(self):
        return self.KEYS.keys()

    def __getitem__(self, k):
        from bmp import functional as Fn
        return Fn.NFP_PATHS[self.KEYS[k]]


@pytest.fixture
def table_on(monkeypatch):
    from bmp import functional as Fn
    return H.force_on(monkeypatch, Fn.NFP_TABLE_DEFAULT)


def _table(name):
    """Host EncBatch of a table: this family's store on the three tables, the harness's dense four-block tile."""
    return H.table("dense") if name == "dense" else NT.table(name)


def _host_nd(name):
    from bmp.nfp import nfp_derived
    return nfp_derived(_table(name).pb_enc, enc=True)


def _on_device(name):
    """(the table's batch on the device, its derived data from the device kernels)."""
    from bmp.nfp import nfp_derived
    pb = to_dev(_table(name).pb_enc)
    assert pb.n_rows < 800 and pb.mt_row0 is not None
    nd, hd = nfp_derived(pb, enc=True), _host_nd(name)
    for k in ("self_w", "deg_class", "bwd_w", "deg_cnt"):
        assert torch.equal(nd[k].cpu(), hd[k]), k
    if name != "dense":
        NT.check_classes(_table(name).pb_enc, hd)
    return pb, nd


# ---- one layer and one readout on the tables, against the row-wise kernels and the float64 restatement ----
LAYER_NAMES, LAYER_LABELS = ("h", "WT", "B"), ("out", "dh", "dWT", "dB")
READ_NAMES, READ_LABELS = ("h", "WoT", "bo"), ("g", "dh", "dWoT", "dbo")
LAYER_CASES = (("own", 64), ("shared", 64), ("seven", 64), ("dense", 64), ("own", 128))
READ_CASES = (("own", 64, 8), ("shared", 64, 128), ("seven", 64, 8), ("dense", 64, 128), ("own", 128, 128))


def _operands(name, d, o):
    """Float64 operands on table ``name`` in the kernels' layouts, drawn once, and the two cotangents."""
    key = ("ops", name, d, o)
    if key not in _CACHE:
        pb = _table(name).pb_enc
        N, U = pb.n_rows, pb.n_mols
        g = torch.Generator().manual_seed(500 + d + o + len(name))
        r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
        _CACHE[key] = dict(h=r(N, d), WT=r(7, d, d) / d ** 0.5, B=0.3 * r(d), WoT=r(d, o) / d ** 0.5, bo=0.3 * r(o), c=r(N, d),
                           cg=r(U, o))
    return _CACHE[key]


def _ref_layer(name, d, dtype=torch.float64):
    """out = sigmoid(fv . W_class + B), fv = self_w h + the type-blind neighbour sum, on the table's rows; the rows of no
    gradient (nd["bwd_w"] == 0: the dead rows) take no cotangent.  (out, {operand: gradient})."""
    pb, nd, o = _table(name).pb_enc, _host_nd(name), _operands(name, d, 8)
    q = {k: o[k].to(dtype).clone().requires_grad_(True) for k in LAYER_NAMES}
    N = pb.n_rows
    src = (pb.csr_col >> 2).long()
    dst = torch.repeat_interleave(torch.arange(N), (pb.csr_ptr[1:] - pb.csr_ptr[:-1]).long())
    fv = (nd["self_w"].to(dtype)[:, None] * q["h"]).index_add(0, dst, pb.csr_val.to(dtype)[:, None] * q["h"][src])
    Ws = torch.cat((torch.zeros(1, d, d, dtype=dtype), q["WT"]))
    out = torch.sigmoid(torch.einsum("nk,nkc->nc", fv, Ws[nd["deg_class"].long()]) + q["B"])
    (out * o["c"].to(dtype) * nd["bwd_w"].to(dtype)[:, None]).sum().backward()
    return out.detach(), {k: q[k].grad for k in LAYER_NAMES}


def _ref_readout(name, d, o_):
    pb, o = _table(name).pb_enc, _operands(name, d, o_)
    q = {k: o[k].clone().requires_grad_(True) for k in READ_NAMES}
    live = pb.row_mol.long() >= 0
    s = torch.softmax(q["h"] @ q["WoT"] + q["bo"], dim=1) * pb.row_w.double()[:, None]
    g = torch.zeros(pb.n_mols, o_, dtype=torch.float64).index_add(0, pb.row_mol.long()[live], s[live])
    (g * o["cg"]).sum().backward()
    return g.detach(), {k: q[k].grad for k in READ_NAMES}


def _restatement(kind, *case):
    key = ("ref", kind) + case
    if key not in _CACHE:
        _CACHE[key] = (_ref_layer if kind == "layer" else _ref_readout)(*case)
    return _CACHE[key]


def _args(o, names, grad):
    return {k: o[k].float().to(dev()).requires_grad_(grad) for k in names}


def _run_layer(name, d, pb, nd, fused):
    from bmp import functional as Fn
    o = _operands(name, d, 8)
    q = _args(o, LAYER_NAMES, True)
    out = Fn.NFPLayerFn.apply(q["h"], q["WT"], q["B"], pb, nd, fused)
    (out * o["c"].float().to(dev()) * nd["bwd_w"][:, None]).sum().backward()
    return out.detach(), {k: q[k].grad for k in LAYER_NAMES}


def _run_readout(name, d, o_, pb, fused):
    from bmp import functional as Fn
    o = _operands(name, d, o_)
    q = _args(o, READ_NAMES, True)
    g = Fn.NFPReadoutFn.apply(q["h"], q["WoT"], q["bo"], pb, None, fused)
    (g * o["cg"].float().to(dev())).sum().backward()
    return g.detach(), {k: q[k].grad for k in READ_NAMES}


@pytest.mark.parametrize("name,d", LAYER_CASES)
def test_table_layer_against_rows_and_restatement(name, d, table_on):
    Fn = table_on
    pb, nd = _on_device(name)
    q = _args(_operands(name, d, 8), LAYER_NAMES, False)
    H.step_against_composed_and_restatement(
        _paths(), lambda fused: _run_layer(name, d, pb, nd, fused), _restatement("layer", name, d), f"nfp layer {name} d={d}",
        LAYER_NAMES, LAYER_LABELS, [lambda: Fn.NFPLayerFn.apply(q["h"], q["WT"], q["B"], pb, nd, True)])     # forward only: null fv


@pytest.mark.parametrize("name,d,o", READ_CASES)
def test_table_readout_against_rows_and_restatement(name, d, o, table_on):
    Fn = table_on
    pb, _nd = _on_device(name)
    q = _args(_operands(name, d, o), READ_NAMES, False)
    fz, _comp = H.step_against_composed_and_restatement(
        _ReadoutPaths(), lambda fused: _run_readout(name, d, o, pb, fused), _restatement("readout", name, d, o),
        f"nfp readout {name} d={d} o={o}", READ_NAMES, READ_LABELS,
        [lambda: Fn.NFPReadoutFn.apply(q["h"], q["WoT"], q["bo"], pb, None, True)])
    # ... and accumulated in place onto the readout of the layers before it
    g_prev = torch.full_like(fz[0], 0.25)
    with torch.no_grad():
        g = Fn.NFPReadoutFn.apply(q["h"], q["WoT"], q["bo"], pb, g_prev, True)
    assert g.data_ptr() == g_prev.data_ptr() and torch.equal(g, fz[0] + 0.25)


# ---- through the C ABI ----
def _weights(d, o, seed):
    from bmp.functional import pack_k4
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    W = rnd(7, d, d) / d ** 0.5                        # [class][out x in], the reference layout
    Wo = rnd(o, d) / d ** 0.5
    pk = lambda X: torch.stack([pack_k4(X[k]) for k in range(7)])
    return dict(WTp=pk(W.transpose(1, 2).contiguous()), Wnp=pk(W), B=0.3 * rnd(d), WoTp=pack_k4(Wo.t().contiguous()), Wonp=pack_k4(Wo),
                bo=0.3 * rnd(o))


def _entry(kind, entry, direction):
    from bmp import _lib
    name = f"bmp_nfp_{kind}_{entry}_{direction}"
    return getattr(_lib.lib(), name), name


def _abi_layer_fwd(entry, d, n_tiles, h, csr, self_w, cls, W, fv, out, tab=()):
    from bmp._lib import check, ptr, stream
    f, name = _entry("layer", entry, "fwd")
    check(f(ptr(h), n_tiles, d, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ptr(self_w), ptr(cls), ptr(W["WTp"]), ptr(W["B"]), ptr(fv),
            ptr(out), *tab, stream()), name)


def _abi_layer_bwd(entry, d, n_tiles, dout, out, csrT, self_w, cls, bwd_w, W, dpre, dh, tab=()):
    from bmp._lib import check, ptr, stream
    f, name = _entry("layer", entry, "bwd")
    check(f(ptr(dout), ptr(out), n_tiles, d, ptr(csrT[0]), ptr(csrT[1]), ptr(csrT[2]), ptr(self_w), ptr(cls), ptr(bwd_w), ptr(W["Wnp"]),
            ptr(dpre), ptr(dh), *tab, stream()), name)


def _abi_readout_fwd(entry, d, o, n_tiles, h, W, row_w, row_mol, s, g, acc, tab=()):
    from bmp._lib import check, ptr, stream
    f, name = _entry("readout", entry, "fwd")
    check(f(ptr(h), n_tiles, d, o, ptr(W["WoTp"]), ptr(W["bo"]), ptr(row_w), ptr(row_mol), ptr(s), ptr(g), acc, *tab, stream()), name)


def _abi_readout_bwd(entry, d, o, n_tiles, N, dg, h, s, W, row_w, row_mol, dh, dWT, db, ws, tab=()):
    from bmp._lib import check, ptr, stream
    f, name = _entry("readout", entry, "bwd")
    check(f(ptr(dg), ptr(h), ptr(s), n_tiles, d, o, ptr(W["Wonp"]), ptr(row_w), ptr(row_mol), ptr(dh), ptr(dWT), ptr(db), ptr(ws),
            ws.numel(), *tab, stream()), name)


def _readout_ws(N, d, o, fill=0.0):
    from bmp import _lib
    return torch.full((int(_lib.lib().bmp_nfp_readout_bwd_ws_floats(N, d, o)),), fill, device=dev())


@pytest.mark.parametrize("d,o", [(64, 8), (128, 128)])
def test_table_of_whole_tiles_is_the_whole_tile_kernel_bit_for_bit(d, o):
    """Every table entry a four-block tile at 128 t, on the per-instance batch of the "hand" world (whole tiles, every degree
    class): the products run in the same order, so every written array is bit-identical."""
    from bmp import packed
    from bmp.nfp import nfp_derived
    mols, I1, I2 = NT.world_molecules("hand")
    pb = packed.pack_from_store(packed.MolStore(mols), [I1, I2], device=dev())
    nd = nfp_derived(pb)
    assert set(nd["deg_class"].cpu().tolist()) == set(range(8))
    N, nt, U = pb.n_rows, pb.n_tiles, pb.n_mols
    csr, csrT = (pb.csr_ptr, pb.csr_col, pb.csr_val), (pb.csrT_ptr, pb.csrT_col, pb.csrT_val)
    W = _weights(d, o, 40 + d)
    g_ = torch.Generator().manual_seed(41)
    rnd = lambda *s: torch.randn(*s, generator=g_).to(dev())
    h, dout, dg = rnd(N, d), rnd(N, d), rnd(U, o)

    def run(entry, tab):
        z = lambda *s: torch.zeros(*s, device=dev())
        fv, out, dpre, dh, s, g, rdh, dWT, db = z(N, d), z(N, d), z(N, d), z(N, d), z(N, o), z(U, o), z(N, d), z(d, o), z(o)
        ws = _readout_ws(N, d, o)
        _abi_layer_fwd(entry, d, nt, h, csr, nd["self_w"], nd["deg_class"], W, fv, out, tab)
        _abi_layer_bwd(entry, d, nt, dout, out, csrT, nd["self_w"], nd["deg_class"], nd["bwd_w"], W, dpre, dh, tab)
        _abi_readout_fwd(entry, d, o, nt, out, W, pb.row_w, pb.row_mol, s, g, 0, tab)
        _abi_readout_bwd(entry, d, o, nt, N, dg, out, s, W, pb.row_w, pb.row_mol, rdh, dWT, db, ws, tab)
        torch.cuda.synchronize()
        return dict(fv=fv, out=out, dpre=dpre, dh=dh, s=s, g=g, readout_dh=rdh, dz=ws[:N * o].clone(), dWoT=dWT, dbo=db)

    H.whole_tiles_bit_for_bit(pb, run, f"nfp d={d} o={o}", ("out", "dh", "g", "readout_dh", "dWoT"))


def _stride_rows(ns, live):
    """The per-row data of ``H.stride_case(ns)`` under the per-instance convention -- chains: the ends have class 2, the others
    3; a pad row of multiplicity P_PAD behind each -- with the dead rows as nothing may read them: NaN in the float arrays, a
    class and a molecule that would show in the ints."""
    N = H.STRIDE_ROWS
    self_w, row_w = torch.full((N,), float("nan")), torch.full((N,), float("nan"))
    cls, row_mol = torch.full((N,), 5, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    for t, n in enumerate(ns):
        a = 128 * t
        self_w[a:a + n] = 1.0; self_w[a + n] = 0.0
        row_w[a:a + n] = 1.0; row_w[a + n] = P_PAD
        cls[a:a + n] = 3; cls[a] = cls[a + n - 1] = 2; cls[a + n] = 0
        row_mol[a:a + n + 1] = t
        row_mol[a + n + 1:a + 32 * ((n + 1 + 31) // 32)] = -1            # the dead rows inside the last live block
        self_w[a + n + 1:a + 32 * ((n + 1 + 31) // 32)] = 0.0
        row_w[a + n + 1:a + 32 * ((n + 1 + 31) // 32)] = 0.0
        cls[a + n + 1:a + 32 * ((n + 1 + 31) // 32)] = 0
    lv = live.cpu()
    assert torch.isnan(self_w[~lv]).all() and not torch.isnan(self_w[lv]).any() and (cls[~lv] == 5).all()
    return self_w.to(dev()), cls.to(dev()), row_w.to(dev()), row_mol.to(dev())


@pytest.mark.parametrize("ns", sorted(H.STRIDE_BLOCKS))
def test_fixed_stride_clears_the_dead_rows(ns):
    """Through the C ABI at d = 64, o = 8 on three tiles at stride 128: every output prefilled with NaN, the dead rows of every
    input NaN too (never read), and a 128-row NaN canary behind mt_rows in every written row array.  With tile_stride = 128 the
    rows of the dead blocks are exactly 0 in fv, out, dpre, dh, s, the readout's dh and its dz workspace and no NaN is left
    anywhere, dW_o, db and g included; the live rows equal the dense-row run; the canary stays NaN either way.  The forward with a
    null fv writes the same out."""
    from bmp._lib import ptr
    d, o, N = 64, 8, H.STRIDE_ROWS
    csr, csrT, r0, nb, live = H.stride_case(ns)
    self_w, cls, row_w, row_mol = _stride_rows(ns, live)
    W = _weights(d, o, 77)
    g_ = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g_).to(dev())
    h, dout, dg = H.nan_dead(rnd(N, d), live), H.nan_dead(rnd(N, d), live), rnd(3, o)
    res, extra = {}, {}
    for stride in (128, 0):
        fv, out, dpre, dh, out0, rdh = (H.nan_rows(d) for _ in range(6))
        s = H.nan_rows(o)
        g, dWT, db = (torch.full(shape, float("nan"), device=dev()) for shape in ((3, o), (d, o), (o,)))
        ws = _readout_ws(N, d, o, float("nan"))
        tab = (ptr(r0), ptr(nb), N, stride)
        _abi_layer_fwd("table", d, 3, h, csr, self_w, cls, W, fv, out, tab)
        _abi_layer_fwd("table", d, 3, h, csr, self_w, cls, W, None, out0, tab)          # forward only: the same out, no fv
        torch.cuda.synchronize()
        assert torch.equal(out0[:N][live], out[:N][live]) and torch.isnan(out0[N:]).all()
        assert (out0[:N][~live] == 0).all() if stride else torch.isnan(out0[:N][~live]).all()
        res[stride] = dict(fv=fv, out=out.clone())
        out[:N] = H.nan_dead(out[:N], live)                                             # the inputs of what follows: dead rows NaN again
        _abi_layer_bwd("table", d, 3, dout, out, csrT, self_w, cls, row_w, W, dpre, dh, tab)
        _abi_readout_fwd("table", d, o, 3, out, W, row_w, row_mol, s, g, 0, tab)
        torch.cuda.synchronize()
        res[stride].update(dpre=dpre, dh=dh, s=s.clone())
        s[:N] = H.nan_dead(s[:N], live)
        # (h is the weight gradient's operand only, a GEMM over all rows: the layer's own output, dead rows as it left them)
        _abi_readout_bwd("table", d, o, 3, N, dg, res[stride]["out"], s, W, row_w, row_mol, rdh, dWT, db, ws, tab)
        torch.cuda.synchronize()
        res[stride].update(readout_dh=rdh)
        extra[stride] = dict(g=g, dz=ws[:N * o].view(N, o).clone(), dWoT=dWT, dbo=db)
    H.fixed_stride_clears_the_dead_rows(res, live, ("out", "dh", "s", "readout_dh"))
    dz, dz0 = extra[128]["dz"], extra[0]["dz"]
    assert (dz[~live] == 0).all() and torch.isfinite(dz).all() and torch.equal(dz[live], dz0[live]) and torch.isnan(dz0[~live]).all()
    assert torch.isfinite(extra[128]["g"]).all() and torch.equal(extra[128]["g"], extra[0]["g"]) and extra[128]["g"].abs().max() > 0
    assert torch.isfinite(extra[128]["dWoT"]).all() and torch.isfinite(extra[128]["dbo"]).all() and dz[live].abs().max() > 0
    # the pad rows' softmax counts P_PAD times: g is the sum of s weighted by row_w
    sw = res[128]["s"][:N] * torch.nan_to_num(row_w)[:, None]
    want = torch.stack([sw[128 * t:128 * t + n + 1].sum(dim=0) for t, n in enumerate(ns)])
    close(extra[128]["g"], want, "fixed stride: g vs the weighted sum of s", tol=1e-5)


def test_table_entries_refuse_the_bad_tables():
    d, o, N = 64, 8, H.STRIDE_ROWS
    ns = (20, 70, 120)
    csr, csrT, r0, nb, live = H.stride_case(ns)
    self_w, cls, row_w, row_mol = _stride_rows(ns, live)
    W = _weights(d, o, 78)
    z = lambda *s: torch.zeros(*s, device=dev())
    h, fv, out, dpre, dh, s, g, dWT, db, dg = z(N, d), z(N, d), z(N, d), z(N, d), z(N, d), z(N, o), z(3, o), z(d, o), z(o), z(3, o)
    ws = _readout_ws(N, d, o)
    H.refuses_the_bad_tables(
        r0, nb,
        lambda tab: _abi_layer_fwd("table", d, 3, h, csr, self_w, cls, W, fv, out, tab),
        lambda tab: _abi_layer_bwd("table", d, 3, h, out, csrT, self_w, cls, row_w, W, dpre, dh, tab),
        lambda tab: _abi_readout_fwd("table", d, o, 3, h, W, row_w, row_mol, s, g, 0, tab),
        lambda tab: _abi_readout_bwd("table", d, o, 3, N, dg, h, s, W, row_w, row_mol, dh, dWT, db, ws, tab))


# ---- the derived data on the device ----
def _to_host(pb):
    kw = {f.name: getattr(pb, f.name).cpu() for f in dataclasses.fields(pb) if isinstance(getattr(pb, f.name), torch.Tensor)}
    return dataclasses.replace(pb, **kw, _cache={})


@pytest.mark.parametrize("dedup", [False, True], ids=["instances", "dedup"])
@pytest.mark.parametrize("which", ["hand", "single"])
def test_derived_data_on_the_device_is_the_host_form_bit_for_bit(which, dedup):
    from bmp.nfp import nfp_derived
    _pb, _t, eb, _t2 = H.batches(NT.world(which, dev()), dedup, 5)
    nd, hd = nfp_derived(eb.pb_enc, enc=True), nfp_derived(_to_host(eb.pb_enc), enc=True)
    for k in ("self_w", "deg_class", "bwd_w", "deg_cnt"):
        assert torch.equal(nd[k].cpu(), hd[k]), k
    N, cnt = eb.pb_enc.n_rows, hd["deg_cnt"]
    for k in range(7):
        assert torch.equal(nd["deg_rows"].cpu().view(7, N)[k, :cnt[k]], hd["deg_rows"].view(7, N)[k, :cnt[k]]), k
    assert set(hd["deg_class"].tolist()) == set(range(8))
    rm = eb.pb_enc.row_mol.cpu()
    assert (hd["bwd_w"][rm <= -2] == 1).all() and (hd["self_w"][rm <= -2] == 0).all() and (rm <= -2).any()


# ---- encoder level ----
def _pair_model(attn, d=64, layers=LAYERS):
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    model = build_pair_predictor(encoder="nfp", hidden_dim=d, out_dim=d, n_layers=layers, attn=attn).to(dev())
    dr = O._Draw(21, torch.float64, 0.1)
    if attn == "nie":
        O.init_nie(dr, "attn/", d, d, 8)
    O.init_mlp(dr, "mlp/", 2 * d, 1, (32, 16))
    p = dict(dr.p)
    p.update(NR.make_nfp_params(60, d, d, layers, prefix="graph_conv/"))
    load_param_dict(model, p)
    return model


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
@pytest.mark.parametrize("which", ["hand", "single"])
def test_encoder_trains_in_the_encoder_layout(which, attn, dedup, n_cu, table_on, monkeypatch):
    """With a co-attention the gradient of the seven biases of every layer arrives, in part, through the encoder layout's pad
    rows (row_w == 0 there): it is wrong where the layer backward tests row_w and not the liveness weight.  Without one nobody
    reads the atom array: no EncRowsFn runs."""
    from bmp import enclayout
    copies, forward = [], enclayout.EncRowsFn.forward
    monkeypatch.setattr(enclayout.EncRowsFn, "forward", staticmethod(lambda ctx, h, eb: copies.append(1) or forward(ctx, h, eb)))
    model = _pair_model(attn)
    assert model.training
    inst, enc = H.encoder_layout_against_per_instance(
        NT.world(which, dev()), model, _paths(), f"nfp {which} attn={attn} dedup={dedup} n_cu={n_cu}", dedup, n_cu, H.fused(LAYERS),
        atoms=model.graph_conv.get_atom_array if attn else None, nonzero="graph_conv/layers")
    assert len(copies) == (1 if attn else 0), copies
    if attn is None:
        assert model.graph_conv.atoms is None
    biases = [k for k in enc["grads"] if "/graph_linears/" in k and k.endswith("/b")]
    assert len(biases) == 7 * LAYERS
    for k in biases:
        assert inst["grads"][k].abs().max() > 0
        close(enc["grads"][k], inst["grads"][k], f"nfp {which} attn={attn} dedup={dedup}: grad {k} vs per-instance", tol=1e-5)
    again = H.pair_run(model, *H.batches(NT.world(which, dev()), dedup, n_cu)[2:])       # two identical runs: bit-equal gradients
    assert all(torch.equal(again["grads"][k], enc["grads"][k]) for k in enc["grads"])


def test_paths_follow_the_switch(monkeypatch):
    from bmp import functional as Fn
    H.paths_follow_the_switch(monkeypatch, NT.world("hand", dev()), _pair_model(None), _paths(), Fn.NFP_TABLE_DEFAULT, 64, LAYERS)


# ---- the fixed-shape batch ----
def _static_model():
    from bmp.nfp import NFP
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    torch.manual_seed(5)
    enc = NFP(out_dim=16, hidden_dim=64, n_layers=LAYERS)
    return GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev())


def test_static_batch_eager_step_equals_the_packed_step(table_on):
    H.static_eager_step_equals_the_packed_step(_static_model(), _paths(), LAYERS, "nfp")


def test_fit_runs_an_nfp_model_in_every_layout(table_on):
    from bmp.predictor import build_pair_predictor
    H.fit_runs_in_every_layout(_paths(), lambda: build_pair_predictor(encoder="nfp", hidden_dim=64, out_dim=32, n_layers=2, attn="nie",
                                                                     head=4), "nfp")


def test_static_batch_recorded_step_replays_on_the_table_kernels(table_on):
    H.static_recorded_step_replays_on_the_table_kernels(_static_model, _paths(), "nfp")
