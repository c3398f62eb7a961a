"""The d = 32 fuse-gate / simple-gate step on a TILE TABLE (csrc/bmp_gate_small_table.hip) and the gated encoders in the encoder
layout, under de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (tests/ggate_ref.py), 1e-5 between two
float32 forms of the same step (test_gpu_static_batch.py, test_gpu_enclayout.py at full size), 1e-4 for parameters after several
replayed steps (test_gpu_static_batch.py).  Every case is a few hundred rows at d = 32.

The tables, the pair world and the bodies shared with the other table families: tests/table_harness.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggate_ref as G                                  # noqa: E402
import table_harness as H                              # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from parity_util import close                          # noqa: E402
from test_gpu_ops import dev                           # noqa: E402

T = torch.from_numpy
D = 32
KIND = {"fuse": 0, "gate": 1}
NAMES = ("h", "WT", "bE", "AU", "bU")
LABELS = ("hout", "dh", "dWT", "dbE", "dAU", "dbU")
_CACHE = {}


def _paths():
    from bmp import functional as Fn
    return Fn.GATE_PATHS


def _operands(kind, name):
    """Float64 operands of one step on table ``name`` in the kernel's layouts, drawn once: h, WT, bE, AU, bU, keep, cotangent."""
    key = ("ops", kind, name)
    if key not in _CACHE:
        N = H.table(name).pb_enc.n_rows
        g = torch.Generator().manual_seed(100 + KIND[kind])
        r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
        nu = (3 if kind == "fuse" else 1) * D
        keep = ((torch.rand(N, D, generator=g) >= 0.3).double() / 0.7) if kind == "fuse" else None
        _CACHE[key] = dict(h=r(N, D), WT=0.5 * r(4 * D, D) / D ** 0.5, bE=0.3 * r(4, D), AU=r(2 * D, nu) / (2 * D) ** 0.5,
                           bU=0.3 * r(nu), keep=keep, c=r(N, D))
    return _CACHE[key]


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
        _g, h = G.forward(kind, p, np.arange(N)[None], H.dense_adj(H.table(name).pb_enc), 1, keep=keep)
        (h[0] * o["c"]).sum().backward()
        _CACHE[key] = (h[0].detach(), {k: q[k].grad for k in NAMES})
    return _CACHE[key]


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


@pytest.mark.parametrize("name", ["own", "shared", "seven"])
@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_table_step_against_composed_and_restatement(kind, name):
    from bmp import functional as Fn
    pb = H.table_on_device(name)
    o = _operands(kind, name)
    args = [o[k].float().to(dev()) for k in NAMES]
    keep = None if o["keep"] is None else o["keep"].float().to(dev())
    H.step_against_composed_and_restatement(_paths(), lambda fused: _run_step(kind, name, pb, fused), _restatement(kind, name),
                                            f"{name} {kind}", NAMES, LABELS, [lambda: Fn.GateStepFn.apply(*args, keep, pb, KIND[kind])])


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_fixed_stride_clears_the_dead_rows(kind):
    """Through the C ABI on tiles of 1, 2 and 3 live blocks: every output prefilled with NaN, the inputs' dead rows NaN too (never
    read); the checks are table_harness.fixed_stride_clears_the_dead_rows's, the live rows bit-equal to tile_stride = 0."""
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    from bmp.functional import pack_k4
    L = _lib.lib()
    (cp, cc, cv), (tp, tc, tv), r0, nb, live = H.stride_case((20, 40, 70))
    N, nu, k = H.STRIDE_ROWS, (3 if kind == "fuse" else 1) * D, KIND[kind]
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    h, dhout = H.nan_dead(rnd(N, D), live), H.nan_dead(rnd(N, D), live)
    keep = H.nan_dead((torch.rand(N, D, generator=g) >= 0.3).float().to(dev()) / 0.7, live) if kind == "fuse" else None
    WT, bE, AU, bU = 0.1 * rnd(4 * D, D), 0.3 * rnd(4, D), 0.1 * rnd(2 * D, nu), 0.3 * rnd(nu)
    WTp, AUp, Wnp, Unp = pack_k4(WT), pack_k4(AU), pack_k4(WT.t()), pack_k4(AU.t())

    def fwd(m, act, hout, tab):
        check(L.bmp_ggnn_gate_step_small_table_fwd(k, ptr(h), 3, D, ptr(cp), ptr(cc), ptr(cv), ptr(WTp), ptr(bE), ptr(AUp), ptr(bU),
                                                   ptr(keep), ptr(m), ptr(act), ptr(hout), *tab, stream()),
              "bmp_ggnn_gate_step_small_table_fwd")

    def bwd(m, act, dh, gda, tab):
        check(L.bmp_ggnn_gate_step_small_table_bwd(k, ptr(dhout), ptr(h), ptr(m), ptr(act), ptr(keep), 3, D, ptr(tp), ptr(tc), ptr(tv),
                                                   ptr(Wnp), ptr(Unp), ptr(dh), ptr(gda), *tab, stream()),
              "bmp_ggnn_gate_step_small_table_bwd")

    res = {}
    for stride in (128, 0):
        m, act, hout, dh, gda = (H.nan_rows(n) for n in (D, nu, D, D, 4 * D + nu))
        tab = (ptr(r0), ptr(nb), N, stride)
        fwd(m, act, hout, tab)
        bwd(m, act, dh, gda, tab)
        torch.cuda.synchronize()
        res[stride] = dict(m=m, act=act, hout=hout, dh=dh, gda=gda)
    H.fixed_stride_clears_the_dead_rows(res, live, ("hout", "gda"))
    hout = torch.empty(N, D, device=dev())
    H.refuses_the_bad_tables(r0, nb, lambda tab: fwd(None, None, hout, tab), lambda tab: bwd(m, act, dh, gda, tab))


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_table_tile_with_more_entries_than_the_staged_csr(kind):
    """One four-block table tile whose CSR does not fit the staging in LDS: both directions gather from global memory."""
    pb = H.table_on_device("dense")
    fused, took = H.took(_paths(), lambda: _run_step(kind, "dense", pb, True))
    assert took == H.FUSED, took
    H.compare(fused, _run_step(kind, "dense", pb, False), f"dense table tile {kind} vs composed", 1e-5, NAMES, LABELS)


# ---- encoder level: the 9-molecule, 13-pair heavy-repetition set of test_gpu_enclayout.py ----
LAYERS = 3


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
        w = H.world("synthetic")
        q = {k: v.clone().requires_grad_() for k, v in _pair_params(kind, attn).items()}
        out = [G.forward(kind, q, *synth.concat_mols([w.store[k] for k in idx]), LAYERS, tying=False, prefix="graph_conv/")
               for idx in (w.I1, w.I2)]
        g1, g2 = out[0][0], out[1][0]
        if attn == "nie":
            g1, g2 = O.nie_coattention(q, out[0][1], out[1][1], "tanh", prefix="attn/")
        y = O.mlp_forward(q, torch.cat((g1, g2), dim=-1), 2)
        names = sorted(q)
        gr = torch.autograd.grad(O.sigmoid_cross_entropy(y, T(H.LAB)), [q[n] for n in names], allow_unused=True)
        _CACHE[key] = dict(y=y.detach(), g1=g1.detach(), g2=g2.detach(),
                           grads={n: (x if x is not None else torch.zeros_like(q[n])) for n, x in zip(names, gr)})
    return _CACHE[key]


def _pair_model(kind, attn, d=D):
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    model = build_pair_predictor(encoder="ggnn-" + kind, hidden_dim=d, out_dim=d, n_layers=LAYERS, weight_tying=False, attn=attn).to(dev())
    load_param_dict(model, _pair_params(kind, attn, d))
    return model


def _in_the_encoder_layout(model, tag, dedup, n_cu, **kw):
    return H.encoder_layout_against_per_instance(H.world("synthetic"), model, _paths(), tag, dedup, n_cu, H.fused(LAYERS),
                                                 atoms=model.graph_conv.get_atom_array, **kw)


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
def test_gate_encoder_trains_in_the_encoder_layout(attn, dedup, n_cu):
    model = _pair_model("gate", attn)
    assert model.training
    tag = f"gate attn={attn} dedup={dedup} n_cu={n_cu}"
    _inst, enc = _in_the_encoder_layout(model, tag, dedup, n_cu)
    ref = _pair_reference("gate", attn)
    for k in ("y", "g1", "g2"):
        close(enc[k], ref[k], f"{tag}: {k} vs float64")
    assert sorted(enc["grads"]) == sorted(ref["grads"])
    for name, gr in enc["grads"].items():
        floor = 1e-6                                     # the floors of test_gpu_enclayout.py's oracle comparison
        if name == "attn/energy_layer/b":
            floor = ref["grads"]["attn/energy_layer/V1"].abs().max().item()
        if name.startswith("attn/energy_layers"):
            floor = 1e-4 * max(v.abs().max().item() for k, v in ref["grads"].items() if k.startswith("attn/"))
        close(gr, ref["grads"][name], f"{tag}: grad {name} vs float64", floor=floor)


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
def test_fuse_encoder_evaluates_in_the_encoder_layout_and_refuses_to_train_there(attn, dedup, n_cu):
    from bmp import ggnn_gate
    model = _pair_model("fuse", attn).eval()
    tag = f"fuse attn={attn} dedup={dedup} n_cu={n_cu}"
    with torch.no_grad():
        _inst, enc = _in_the_encoder_layout(model, tag, dedup, n_cu, backward=False)
    ref = _pair_reference("fuse", attn)
    for k in ("y", "g1", "g2"):
        close(enc[k], ref[k], f"{tag}: {k} vs float64")
    model.train()
    with pytest.raises(NotImplementedError) as e:
        model(H.batches(H.world("synthetic"), dedup, n_cu)[2])
    assert str(e.value) == "encode_rows: " + ggnn_gate.FUSE_TRAIN_LAYOUT_REASON


@pytest.mark.parametrize("kind", ["fuse", "gate"])
def test_width_64_on_a_table_batch_stays_composed(kind):
    """The d = 64 / 128 kernels take no table: the encoder layout runs the composed operators there, with the per-instance
    result."""
    model = _pair_model(kind, None, d=64).eval()
    _in_the_encoder_layout(model, f"d = 64 {kind} table batch", True, 5, took_enc={"fused": 0, "composed": LAYERS})


# ---- the fixed-shape batch ----
def _static_model(kind):
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.ggnn_gate import FuseGGNN, GateGGNN
    torch.manual_seed(5)
    enc = (FuseGGNN if kind == "fuse" else GateGGNN)(out_dim=16, hidden_dim=D, n_layers=3, weight_tying=False)
    return GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev())


def test_static_batch_eager_fuse_step_equals_the_packed_step():
    """Training mode with the masks given (table_harness.static_eager_step_equals_the_packed_step)."""
    H.static_eager_step_equals_the_packed_step(_static_model("fuse"), _paths(), 3, "fuse", masks=(D, 0.05))


def test_static_batch_recorded_gate_step_replays_on_the_table_kernels():
    H.static_recorded_step_replays_on_the_table_kernels(lambda: _static_model("gate"), _paths(), "gate")
