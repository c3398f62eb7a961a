"""The self-loop GGNN step on a TILE TABLE (csrc/bmp_loop_table.hip) and the encoders of bmp/ggnn_dev.py in the encoder layout,
under de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (tests/ggdev_ref.py), 1e-5 between two
float32 forms of the same step, 1e-4 for parameters after several replayed steps (test_gpu_static_batch.py).  The store, the
three tables and the shared bodies are tests/table_harness.py's (the tables' properties: tests/test_ggdev_enc_build.py); every
case is under 800 rows at d = 64, one repeats at d = 128.  The tests that go through ``loop_step`` force ``LOOP_TABLE_DEFAULT`` on: they do not depend on
the measured default."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggdev_ref as R                                  # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from test_gpu_ops import dev, to_dev                   # noqa: E402
import table_harness as H                              # noqa: E402

NAMES = ("h", "WT", "bE", "WsT", "bs", "AT", "UcT", "b")
LABELS = ("hout", "dh", "dWT", "dbE", "dWsT", "dbs", "dAT", "dUcT", "db")
LAYERS = 3
_CACHE = {}


def _paths():
    from bmp import functional as Fn
    return Fn.LOOP_PATHS


@pytest.fixture
def table_on(monkeypatch):
    from bmp import functional as Fn
    return H.force_on(monkeypatch, Fn.LOOP_TABLE_DEFAULT)


# ---- one step on the three tables ----
def _operands(name, d):
    """Float64 operands of one step on table ``name`` in the kernel's layouts, drawn once, and the cotangent."""
    key = ("ops", name, d)
    if key not in _CACHE:
        N = H.table(name).pb_enc.n_rows
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
        adj = H.dense_adj(H.table(name).pb_enc)
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


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("name,d", [("own", 64), ("shared", 64), ("seven", 64), ("own", 128)])
def test_table_step_against_composed_and_restatement(name, d, first, table_on):
    Fn = table_on
    pb = H.table_on_device(name)
    args = [_operands(name, d)[k].float().to(dev()) for k in NAMES]
    H.step_against_composed_and_restatement(
        _paths(), lambda fused: _run_step(name, d, first, pb, fused), _restatement(name, d, first), f"{name} d={d} first={first}",
        NAMES, LABELS, [lambda: Fn.LoopStepFn.apply(*args, pb, first),     # forward-only evaluation: null m / rz / c
                        lambda: Fn.loop_step(*args, first, pb)])           # ... and what loop_step picks with the switch on


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
    pb = to_dev(R.data("fixture")["pb"])
    N, nt = pb.n_rows, pb.n_tiles
    csr, csrT = (pb.csr_ptr, pb.csr_col, pb.csr_val), (pb.csrT_ptr, pb.csrT_col, pb.csrT_val)
    W = _weights(d, 40 + d)
    g = torch.Generator().manual_seed(41)
    h, dhout = torch.randn(N, d, generator=g).to(dev()), torch.randn(N, d, generator=g).to(dev())

    def run(entry, tab):
        z = lambda n: torch.zeros(N, n, device=dev())
        m, rz, c, hout, dh, gda, rh = z(d), z(2 * d), z(d), z(d), z(d), z(8 * d), (None if first else z(d))
        _abi_fwd(entry, first, d, nt, h, csr, W, m, rz, c, hout, tab)
        _abi_bwd(entry, first, d, nt, dhout, h, rz, c, csrT, W, dh, gda, rh, tab)
        torch.cuda.synchronize()
        return dict(m=m, rz=rz, c=c, hout=hout, dh=dh, gda=gda, rh=rh if rh is not None else z(1))

    H.whole_tiles_bit_for_bit(pb, run, f"d={d} first={first}", ("hout", "gda"),
                              contracted={k for dd, ff, k in CONTRACTED if (dd, ff) == (d, first)})


@pytest.mark.parametrize("first", [True, False])
def test_fixed_stride_clears_the_dead_rows(first):
    """Through the C ABI at d = 64: every output prefilled with NaN, the dead rows of h, dhout, rz and c NaN too (never read), and a
    128-row NaN canary behind mt_rows in every written array.  With tile_stride = 128 the rows of the dead blocks are exactly 0
    after forward and backward and the live rows finite and bit-equal to tile_stride = 0, which leaves the dead rows NaN; the
    canary stays NaN either way."""
    from bmp._lib import ptr
    d, N = 64, H.STRIDE_ROWS
    csr, csrT, r0, nb, live = H.stride_case((20, 70, 120))
    W = _weights(d, 77)
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    h, dhout = H.nan_dead(rnd(N, d), live), H.nan_dead(rnd(N, d), live)
    res = {}
    for stride in (128, 0):
        m, rz, c, hout, dh, gda = (H.nan_rows(n) for n in (d, 2 * d, d, d, d, 8 * d))
        rh = None if first else H.nan_rows(d)
        tab = (ptr(r0), ptr(nb), N, stride)
        _abi_fwd("table", first, d, 3, h, csr, W, m, rz, c, hout, tab)
        torch.cuda.synchronize()
        out = dict(m=m.clone(), rz_z=rz[:, d:].clone(), c=c.clone(), hout=hout.clone())
        if not first:
            out["rz_r"] = rz[:, :d].clone()
        rz[:N] = H.nan_dead(rz[:N], live); c[:N] = H.nan_dead(c[:N], live)           # the backward's inputs: dead rows NaN again
        _abi_bwd("table", first, d, 3, dhout, h, rz, c, csrT, W, dh, gda, rh, tab)
        torch.cuda.synchronize()
        out.update(dh=dh, gda=gda)
        if not first:
            out["rh"] = rh
        res[stride] = out
    H.fixed_stride_clears_the_dead_rows(res, live, ("hout", "gda"))
    if first:                                            # no r: its half of rz is not written, the da_r block is zeros
        assert torch.isnan(rz[:N][live][:, :d]).all() and (res[0]["gda"][:N][live][:, 5 * d:6 * d] == 0).all()
    hout = torch.empty(N, d, device=dev())
    H.refuses_the_bad_tables(r0, nb, lambda tab: _abi_fwd("table", first, d, 3, h, csr, W, None, None, None, hout, tab),
                             lambda tab: _abi_bwd("table", first, d, 3, dhout, h, rz, c, csrT, W, dh, gda, rh, tab))


# ---- encoder level: pairs of the hand-made store, every molecule on both sides and several times ----
ENC = {"dev": "ggnn-dev", "loop": "ggnn-self-loop"}


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


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
@pytest.mark.parametrize("kind", ["dev", "loop"])
def test_encoders_train_in_the_encoder_layout(kind, attn, dedup, n_cu, table_on):
    w = H.world("hand")
    model = _pair_model(kind, attn)
    assert model.training
    # the atom array handed to the co-attention: the last step's states on the instance rows
    atoms = (lambda: model.graph_conv.get_atom_array(-1)) if kind == "dev" else model.graph_conv.get_atom_array
    H.encoder_layout_against_per_instance(w, model, _paths(), f"{kind} attn={attn} dedup={dedup} n_cu={n_cu}", dedup, n_cu,
                                          H.fused(LAYERS if kind == "loop" else 0), atoms=atoms, atoms_name="last-step atoms")
    if kind == "dev":
        pb = H.batches(w, dedup, n_cu)[0]
        at_enc = atoms()
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
    w = H.world("hand")
    H.paths_follow_the_switch(monkeypatch, w, _pair_model("loop", None), _paths(), Fn.LOOP_TABLE_DEFAULT, 64, LAYERS)
    pb, t, eb, t2 = H.batches(w, True, 5)
    small = _pair_model("loop", None, d=32)              # hidden 32 has no fused self-loop step: composed either way
    for on in (True, False):
        monkeypatch.setitem(Fn.LOOP_TABLE_DEFAULT, 64, on)
        _r, took = H.took(_paths(), lambda: H.pair_run(small, eb, t2))
        assert took == {"fused": 0, "composed": LAYERS}, (on, took)
        _r, took = H.took(_paths(), lambda: H.pair_run(small, pb, t))
        assert took == {"fused": 0, "composed": LAYERS}, (on, took)


@pytest.mark.parametrize("kind", ["dev", "loop"])
def test_encode_rows_refuses_dropout_in_training_and_concat_hidden(kind):
    from bmp import ggnn_gate
    from bmp.ggnn_dev import DevGGNN, SelfLoopGGNN
    cls = DevGGNN if kind == "dev" else SelfLoopGGNN
    pb, t, eb, t2 = H.batches(H.world("hand"), True, 5)
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
    H.static_eager_step_equals_the_packed_step(_static_model(), _paths(), 3, "self loop")


def test_fit_runs_a_self_loop_model_in_every_layout(table_on):
    from bmp.predictor import build_pair_predictor
    H.fit_runs_in_every_layout(_paths(), lambda: build_pair_predictor(encoder="ggnn-self-loop", hidden_dim=64, out_dim=32, n_layers=2,
                                                                     attn="nie", head=4), "self-loop")


def test_static_batch_recorded_step_replays_on_the_table_kernels(table_on):
    H.static_recorded_step_replays_on_the_table_kernels(_static_model, _paths(), "self-loop")
