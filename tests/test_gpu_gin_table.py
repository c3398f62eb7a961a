"""The GIN layer on a TILE TABLE (csrc/bmp_gin_table.hip) and the GIN encoder (bmp/gin.py) in the encoder layout, under
de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (tests/gin_ref.py), 1e-5 between two
float32 forms of the same layer, 1e-4 for parameters after several replayed steps (test_gpu_static_batch.py).  The store, the
three tables, the pairs, the stride case and the shared bodies are tests/table_harness.py's (the tables' properties:
tests/test_ggdev_enc_build.py); every case is under 800 rows at d = 64, one repeats at d = 128.  The tests that
go through ``gin_layer`` force ``GIN_TABLE_DEFAULT`` on: they do not depend on the measured default."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gin_ref as R                                    # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from parity_util import close                          # noqa: E402
from test_gpu_ops import dev, to_dev                   # noqa: E402
import table_harness as H                              # noqa: E402

NAMES = ("h", "W1T", "b1", "W2T", "b2")
LABELS = ("out", "dh", "dW1T", "db1", "dW2T", "db2")
LAYERS = 3
_CACHE = {}


def _paths():
    from bmp import functional as Fn
    return Fn.GIN_PATHS


@pytest.fixture
def table_on(monkeypatch):
    from bmp import functional as Fn
    return H.force_on(monkeypatch, Fn.GIN_TABLE_DEFAULT)


# ---- one layer on the three tables ----
# (table, d, masked): the generator seed of the case's operands, the first >= 400 at which the restatement alone meets the relu
# kink condition  min |pre64| >= KINK_FACTOR * max |pre32 - pre64|  over the pre-activations of both linears (the elements a given
# mask zeroes excluded: both sides multiply them by an exact 0) with half as much again to spare (a margin of 12: a float32
# restatement that sums in another order still passes the asserted 8).  ``_kink`` below computes both sides, ``_search_seeds`` is
# the search; both run on the CPU.  Beside each: the margin min |pre64| / max |pre32 - pre64|.
SEEDS = {
    ("own", 64, False): 404,  # 15 x
    ("own", 64, True): 401,  # 15 x
    ("shared", 64, False): 409,  # 22 x
    ("shared", 64, True): 401,  # 37 x
    ("seven", 64, False): 400,  # 53 x
    ("seven", 64, True): 400,  # 87 x
    ("own", 128, False): 447,  # 12 x
    ("own", 128, True): 408,  # 12 x
}
SEED_MARGIN = 1.5                                      # the search's: KINK_FACTOR * SEED_MARGIN
CASES = (("own", 64), ("shared", 64), ("seven", 64), ("own", 128))
P_DROP = 0.5


def _operands(name, d, masked, seed=None):
    """Float64 operands of one layer on table ``name`` in the kernel's layouts, drawn once, the mask and the cotangent."""
    key = ("ops", name, d, masked, seed)
    if key not in _CACHE:
        N = H.table(name).pb_enc.n_rows
        g = torch.Generator().manual_seed(SEEDS[(name, d, masked)] if seed is None else seed)
        r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
        o = dict(h=r(N, d), W1T=r(d, d) / d ** 0.5, b1=0.3 * r(d), W2T=r(d, d) / d ** 0.5, b2=0.3 * r(d), c=r(N, d))
        o["keep"] = (torch.rand(N, d, generator=g) >= P_DROP).double() * (1.0 / (1.0 - P_DROP)) if masked else None
        _CACHE[key] = o
    return _CACHE[key]


def _ref_layer(o, adj, d, dtype, backward=True):
    """tests/gin_ref.py's ``gin_forward`` on the table's rows as one dense molecule of N positions whose atom ids are its row
    numbers; the leaves are the kernel-layout operands, so their gradients come out in the kernel's layouts.
    (out, [pre-activations, the mask's zeros NaN], {operand: gradient})."""
    q = {k: o[k].to(dtype).clone().requires_grad_(backward) for k in NAMES}
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    p = {"embed/W": q["h"], "update_layers/0/linear_g1/W": q["W1T"].t(), "update_layers/0/linear_g1/b": q["b1"],
         "update_layers/0/linear_g2/W": q["W2T"].t(), "update_layers/0/linear_g2/b": q["b2"],
         "readout_layers/0/i_layer/W": z(4, 2 * d), "readout_layers/0/i_layer/b": z(4),
         "readout_layers/0/j_layer/W": z(4, 2 * d), "readout_layers/0/j_layer/b": z(4)}
    N = o["h"].shape[0]
    pre = []
    keep = None if o["keep"] is None else [o["keep"].to(dtype)[None]]
    _g, out = R.gin_forward(p, np.arange(N)[None], adj, True, keep=keep, pre=pre)
    assert len(pre) == 2
    out = out[0]
    if not backward:
        return out.detach(), pre, None
    (out * o["c"].to(dtype)).sum().backward()
    return out.detach(), pre, {k: q[k].grad for k in NAMES}


def _kink(name, d, masked, seed=None):
    """(min |pre64|, max |pre32 - pre64|) of the case's float64 and float32 restatements, a mask's zeros excluded."""
    o = _operands(name, d, masked, seed)
    adj = H.dense_adj(H.table(name).pb_enc)
    with torch.no_grad():
        a64 = _ref_layer(o, adj, d, torch.float64, backward=False)[1]
        a32 = _ref_layer(o, adj, d, torch.float32, backward=False)[1]
    lo, err = float("inf"), 0.0
    for x, y in zip(a64, a32):
        live = ~torch.isnan(x)
        lo = min(lo, x[live].abs().min().item())
        err = max(err, (y.double()[live] - x[live]).abs().max().item())
    return lo, err


def _search_seeds(start=400):
    """Prints the SEEDS table (CPU only)."""
    for name, d in CASES:
        for masked in (False, True):
            for seed in range(start, start + 4000):
                lo, err = _kink(name, d, masked, seed)
                _CACHE.pop(("ops", name, d, masked, seed))
                if lo >= SEED_MARGIN * R.KINK_FACTOR * err:
                    print(f'    ("{name}", {d}, {masked}): {seed},  # {lo / err:.0f} x', flush=True)
                    break


def _restatement(name, d, masked):
    key = ("ref", name, d, masked)
    if key not in _CACHE:
        out, _pre, grads = _ref_layer(_operands(name, d, masked), H.dense_adj(H.table(name).pb_enc), d, torch.float64)
        _CACHE[key] = (out, grads)
    return _CACHE[key]


def _args(o, grad):
    q = {k: o[k].float().to(dev()).requires_grad_(grad) for k in NAMES}
    q["keep"] = None if o["keep"] is None else o["keep"].float().to(dev())
    return q


def _run_layer(name, d, masked, pb, fused):
    """One layer forward and backward in float32 on the device: (out, {operand: gradient})."""
    from bmp import functional as Fn
    o = _operands(name, d, masked)
    q = _args(o, True)
    if fused:
        out = Fn.GinLayerFn.apply(*(q[k] for k in NAMES), q["keep"], pb)
    else:
        out = Fn.gin_layer(*(q[k] for k in NAMES), q["keep"], pb, fused=False)
    (out * o["c"].float().to(dev())).sum().backward()
    return out.detach(), {k: q[k].grad for k in NAMES}


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("name,d", CASES)
def test_table_layer_against_composed_and_restatement(name, d, masked, table_on):
    Fn = table_on
    pb = H.table_on_device(name)
    lo, err = _kink(name, d, masked)
    print(f"[kink] {name} d={d} masked={masked}: min |pre64| {lo:.3e}, max |pre32 - pre64| {err:.3e}, margin {lo / err:.1f} x")
    assert lo >= R.KINK_FACTOR * err, (lo, err)          # no relu of the case sits on its kink at float32 precision
    q = _args(_operands(name, d, masked), False)
    args = [q[k] for k in NAMES] + [q["keep"]]
    H.step_against_composed_and_restatement(
        _paths(), lambda fused: _run_layer(name, d, masked, pb, fused), _restatement(name, d, masked),
        f"{name} d={d} masked={masked}", NAMES, LABELS,
        [lambda: Fn.GinLayerFn.apply(*args, pb),         # forward-only evaluation: null s and t
         lambda: Fn.gin_layer(*args, pb)])               # ... and what gin_layer picks with the switch on


# ---- through the C ABI ----
def _weights(d, seed):
    from bmp.functional import pack_k4
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    W1T, W2T = rnd(d, d) / d ** 0.5, rnd(d, d) / d ** 0.5
    return dict(W1p=pack_k4(W1T), b1=0.3 * rnd(d), W2p=pack_k4(W2T), b2=0.3 * rnd(d), W2np=pack_k4(W2T.t()), W1np=pack_k4(W1T.t()))


def _abi_fwd(entry, d, n_tiles, h, csr, W, keep, s, t, out, tab=()):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    name = f"bmp_gin_layer_{entry}_fwd"
    check(getattr(_lib.lib(), name)(ptr(h), n_tiles, d, ptr(csr[0]), ptr(csr[1]), ptr(csr[2]), ptr(W["W1p"]), ptr(W["b1"]),
                                    ptr(W["W2p"]), ptr(W["b2"]), ptr(keep), ptr(s), ptr(t), ptr(out), *tab, stream()), name)


def _abi_bwd(entry, d, n_tiles, dout, out, keep, t, csrT, W, dp2, dp1, dh, tab=()):
    from bmp import _lib
    from bmp._lib import check, ptr, stream
    name = f"bmp_gin_layer_{entry}_bwd"
    check(getattr(_lib.lib(), name)(ptr(dout), ptr(out), ptr(keep), ptr(t), n_tiles, d, ptr(csrT[0]), ptr(csrT[1]), ptr(csrT[2]),
                                    ptr(W["W2np"]), ptr(W["W1np"]), ptr(dp2), ptr(dp1), ptr(dh), *tab, stream()), name)


# (d, array) whose expression the compiler contracts otherwise in the table instance than in the whole-tile one, held to 1e-5
# (as tests/test_gpu_ggdev_enc.py's): none -- every array of both directions is bit-identical at both widths.
CONTRACTED = set()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("d", [64, 128])
def test_table_of_whole_tiles_is_the_whole_tile_kernel_bit_for_bit(d, masked):
    """Every table entry a four-block tile at 128 t, on the whole-tile batch of tests/gin_ref.py's "fixture" (three tiles): the
    products run in the same order, so every written array is bit-identical."""
    pb = to_dev(R.data("fixture")["pb"])
    N, nt = pb.n_rows, pb.n_tiles
    csr, csrT = (pb.csr_ptr, pb.csr_col, pb.csr_val), (pb.csrT_ptr, pb.csrT_col, pb.csrT_val)
    W = _weights(d, 40 + d)
    g = torch.Generator().manual_seed(41)
    h, dout = torch.randn(N, d, generator=g).to(dev()), torch.randn(N, d, generator=g).to(dev())
    keep = ((torch.rand(N, d, generator=g) >= P_DROP).float() * 2.0).to(dev()) if masked else None

    def run(entry, tab):
        s, t, out, dp2, dp1, dh = (torch.zeros(N, d, device=dev()) for _ in range(6))
        _abi_fwd(entry, d, nt, h, csr, W, keep, s, t, out, tab)
        _abi_bwd(entry, d, nt, dout, out, keep, t, csrT, W, dp2, dp1, dh, tab)
        torch.cuda.synchronize()
        return dict(s=s, t=t, out=out, dp2=dp2, dp1=dp1, dh=dh)

    H.whole_tiles_bit_for_bit(pb, run, f"d={d} masked={masked}", ("out", "dh"), contracted={k for dd, k in CONTRACTED if dd == d})


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
def test_fixed_stride_clears_the_dead_rows(masked):
    """Through the C ABI at d = 64 on tiles of 1, 3 and 4 live blocks at stride 128: every output prefilled with NaN, the dead
    rows of h, keep, dout and (for the backward) out and t NaN too (never read), and a 128-row NaN canary behind mt_rows in every
    written array.  With tile_stride = 128 the rows of the dead blocks are exactly 0 in s, t, out, dp2, dp1 and dh and no NaN is
    left anywhere; the live rows equal the dense-row run (tile_stride = 0, which leaves the dead rows alone) of the same
    molecules; the canary stays NaN either way.  The forward with null s and t writes the same out."""
    from bmp._lib import ptr
    d, N = 64, H.STRIDE_ROWS
    csr, csrT, r0, nb, live = H.stride_case((20, 70, 120))
    W = _weights(d, 77)
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    h, dout = H.nan_dead(rnd(N, d), live), H.nan_dead(rnd(N, d), live)
    keep = H.nan_dead(((torch.rand(N, d, generator=g) >= P_DROP).float() * 2.0).to(dev()), live) if masked else None
    res = {}
    for stride in (128, 0):
        s, t, out, dp2, dp1, dh, out0 = (H.nan_rows(d) for _ in range(7))
        tab = (ptr(r0), ptr(nb), N, stride)
        _abi_fwd("table", d, 3, h, csr, W, keep, s, t, out, tab)
        _abi_fwd("table", d, 3, h, csr, W, keep, None, None, out0, tab)         # forward only: the same out, nothing else written
        torch.cuda.synchronize()
        assert torch.equal(out0[:N][live], out[:N][live]) and torch.isnan(out0[N:]).all()
        assert (out0[:N][~live] == 0).all() if stride else torch.isnan(out0[:N][~live]).all()
        res[stride] = dict(s=s, t=t.clone(), out=out.clone())
        out[:N] = H.nan_dead(out[:N], live); t[:N] = H.nan_dead(t[:N], live)     # the backward's inputs: dead rows NaN again
        _abi_bwd("table", d, 3, dout, out, keep, t, csrT, W, dp2, dp1, dh, tab)
        torch.cuda.synchronize()
        res[stride].update(dp2=dp2, dp1=dp1, dh=dh)
    H.fixed_stride_clears_the_dead_rows(res, live, ("out", "dh"), label=f"masked={masked}")
    # a lone null of s / t is refused, as is every bad table
    s, t, out, dp2, dp1, dh = (torch.empty(N, d, device=dev()) for _ in range(6))
    good = (ptr(r0), ptr(nb), N, 128)
    for s_, t_ in ((s, None), (None, t)):
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_fwd("table", d, 3, h, csr, W, keep, s_, t_, out, good)
    H.refuses_the_bad_tables(r0, nb, lambda tab: _abi_fwd("table", d, 3, h, csr, W, keep, s, t, out, tab),
                             lambda tab: _abi_bwd("table", d, 3, dout, out, keep, t, csrT, W, dp2, dp1, dh, tab))


# ---- encoder level: pairs of the hand-made store, every molecule on both sides and several times ----
def _pair_model(tied, attn, d=64, dropout_ratio=0.0):
    """The pair predictor with a GIN encoder: tied as the trainer builds it (concat_hidden=True, ONE layer and one readout run),
    or untied with LAYERS layers and one readout."""
    from bmp.gin import GIN
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    model = build_pair_predictor(encoder="gin", hidden_dim=d, out_dim=d, n_layers=LAYERS, attn=attn, dropout_ratio=dropout_ratio)
    assert model.graph_conv.concat_hidden and model.graph_conv.weight_tying and model.graph_conv.n_concat == 1
    if not tied:
        model.graph_conv = GIN(out_dim=d, hidden_dim=d, n_layers=LAYERS, dropout_ratio=dropout_ratio, concat_hidden=False,
                               weight_tying=False)
    model = model.to(dev())
    dr = O._Draw(21, torch.float64, 0.1)
    if attn == "nie":
        O.init_nie(dr, "attn/", d, d, 8)
    O.init_mlp(dr, "mlp/", 2 * d, 1, (32, 16))
    p = dict(dr.p)
    p.update(R.make_gin_params(60, d, d, LAYERS, tied, concat_hidden=tied, prefix="graph_conv/"))
    load_param_dict(model, p)
    return model


@pytest.mark.parametrize("dedup,n_cu", [(False, 256), (True, 256), (False, 5), (True, 5)])
@pytest.mark.parametrize("attn", [None, "nie"])
@pytest.mark.parametrize("tied", [True, False], ids=["tied-concat", "untied"])
def test_encoder_trains_in_the_encoder_layout(tied, attn, dedup, n_cu, table_on):
    model = _pair_model(tied, attn)
    ran = 1 if tied else LAYERS
    assert model.training and model.graph_conv.rows_reason() is None and model.graph_conv.n_message_layers == ran
    # (the atom array handed to the co-attention, on the instance rows)
    H.encoder_layout_against_per_instance(H.world("hand"), model, _paths(), f"gin tied={tied} attn={attn} dedup={dedup} n_cu={n_cu}",
                                          dedup, n_cu, H.fused(ran), atoms=model.graph_conv.get_atom_array,
                                          nonzero="graph_conv/update_layers")


def test_encode_rows_refuses_training_dropout_and_concat_of_several_layers(table_on):
    from bmp.ggnn import CONCAT_LAYOUT_REASON, DROPOUT_LAYOUT_REASON
    from bmp.predictor import build_pair_predictor
    pb, t, eb, t2 = H.batches(H.world("hand"), True, 5)
    model = _pair_model(True, None, dropout_ratio=0.5)
    ev, took = H.took(_paths(), lambda: H.pair_run(model.eval(), eb, t2, backward=False))        # evaluation mode: dropout is the identity
    assert took == {"fused": 1, "composed": 0} and torch.isfinite(ev["y"]).all()
    close(ev["y"], H.pair_run(_pair_model(True, None).eval(), eb, t2, backward=False)["y"], "eval() ignores dropout_ratio", tol=1e-5)
    with pytest.raises(NotImplementedError) as e:
        model.train()(eb)
    assert str(e.value) == "encode_rows: " + DROPOUT_LAYOUT_REASON
    cc = build_pair_predictor(encoder="gin", hidden_dim=64, out_dim=64, n_layers=LAYERS, attn=None, weight_tying=False,
                              dropout_ratio=0.0).to(dev())
    assert cc.graph_conv.concat_hidden and cc.graph_conv.n_concat == LAYERS
    with pytest.raises(NotImplementedError) as e:
        cc(eb)
    assert str(e.value) == "encode_rows: " + CONCAT_LAYOUT_REASON
    enc = _pair_model(False, None).graph_conv.eval()
    before = set(vars(enc))
    h, h0 = enc.encode_rows(eb.pb_enc)
    assert h.shape == h0.shape == (eb.pb_enc.n_rows, 64) and torch.isfinite(h).all()
    assert set(vars(enc)) == before and enc.atoms is None     # nothing set that the per-instance call would not set


def test_paths_follow_the_switch(monkeypatch):
    from bmp import functional as Fn
    H.paths_follow_the_switch(monkeypatch, H.world("hand"), _pair_model(False, None), _paths(), Fn.GIN_TABLE_DEFAULT, 64, LAYERS)


# ---- the fixed-shape batch ----
def _static_model(dropout_ratio=0.0):
    from bmp.gin import GIN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    torch.manual_seed(5)
    enc = GIN(out_dim=16, hidden_dim=64, n_layers=LAYERS, dropout_ratio=dropout_ratio, weight_tying=False)
    return GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev())


@pytest.mark.parametrize("masked", [False, True], ids=["no-dropout", "given-masks"])
def test_static_batch_eager_step_equals_the_packed_step(masked, table_on):
    """With masks: training mode at dropout_ratio = 0.5."""
    H.static_eager_step_equals_the_packed_step(_static_model(P_DROP if masked else 0.0), _paths(), LAYERS, "gin",
                                               masks=(64, P_DROP) if masked else None)


def test_fit_runs_a_gin_model_in_every_layout(table_on):
    from bmp.predictor import build_pair_predictor
    H.fit_runs_in_every_layout(_paths(), lambda: build_pair_predictor(encoder="gin", hidden_dim=64, out_dim=32, n_layers=2, attn="nie",
                                                                     head=4, dropout_ratio=0.0), "gin")


def test_static_batch_recorded_step_replays_on_the_table_kernels(table_on):
    H.static_recorded_step_replays_on_the_table_kernels(_static_model, _paths(), "gin")
