"""The GIN layer on a TILE TABLE (csrc/bmp_gin_table.hip) and the GIN encoder (bmp/gin.py) in the encoder layout, under
de-duplication and on the fixed-shape batch.

Tolerances, all the project's: 1e-4 of the tensor's max-abs against the float64 restatement (tests/gin_ref.py), 1e-5 between two
float32 forms of the same layer, 1e-4 for parameters after several replayed steps (test_gpu_static_batch.py).  The store and the
three tables are tests/test_gpu_ggate_enc.py's (their properties: tests/test_ggdev_enc_build.py), the pairs, the stride case and
the batch helpers tests/test_gpu_ggdev_enc.py's; every case is under 800 rows at d = 64, one repeats at d = 128.  The tests that
go through ``gin_layer`` force ``GIN_TABLE_DEFAULT`` on: they do not depend on the measured default."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gin_ref as R                                    # noqa: E402
from oracle import ref_cpu as O                        # noqa: E402
from parity_util import close                          # noqa: E402
from test_gpu_ops import dev, to_dev                   # noqa: E402
from test_gpu_ggate_enc import _dense_adj, _static_world, _table                          # noqa: E402
from test_gpu_ggdev_enc import I1, I2, _atoms_by_molecule, _batches, _pair_run, _stride_case      # noqa: E402

NAMES = ("h", "W1T", "b1", "W2T", "b2")
GRADS = ("dh", "dW1T", "db1", "dW2T", "db2")
LAYERS = 3
_CACHE = {}


@pytest.fixture
def table_on(monkeypatch):
    from bmp import functional as Fn
    for key in Fn.GIN_TABLE_DEFAULT:
        monkeypatch.setitem(Fn.GIN_TABLE_DEFAULT, key, True)
    return Fn


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.GIN_PATHS)
    out = fn()
    return out, {k: Fn.GIN_PATHS[k] - before[k] for k in before}


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
        N = _table(name).pb_enc.n_rows
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
    adj = _dense_adj(_table(name).pb_enc)
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
        out, _pre, grads = _ref_layer(_operands(name, d, masked), _dense_adj(_table(name).pb_enc), d, torch.float64)
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


def _compare(a, b, tag, tol):
    close(a[0], b[0], f"{tag}: out", tol=tol)
    for k, nm in zip(NAMES, GRADS):
        close(a[1][k], b[1][k], f"{tag}: {nm}", tol=tol)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("name,d", CASES)
def test_table_layer_against_composed_and_restatement(name, d, masked, table_on):
    Fn = table_on
    pb = to_dev(_table(name).pb_enc)
    r0, nb = pb.mt_row0.cpu().numpy(), pb.mt_nblk.cpu().numpy()
    cover = np.zeros(pb.n_rows, dtype=int)
    for a, k in zip(r0, nb):
        cover[a:a + 32 * k] += 1
    assert (cover == 1).all() and pb.n_rows < 800        # the table's tiles abut and hold every row once
    lo, err = _kink(name, d, masked)
    print(f"[kink] {name} d={d} masked={masked}: min |pre64| {lo:.3e}, max |pre32 - pre64| {err:.3e}, margin {lo / err:.1f} x")
    assert lo >= R.KINK_FACTOR * err, (lo, err)          # no relu of the case sits on its kink at float32 precision
    ref = _restatement(name, d, masked)
    fused, took = _took(lambda: _run_layer(name, d, masked, pb, True))
    assert took == {"fused": 1, "composed": 0}, took
    comp, took = _took(lambda: _run_layer(name, d, masked, pb, False))
    assert took == {"fused": 0, "composed": 1}, took
    tag = f"{name} d={d} masked={masked}"
    _compare(fused, comp, f"table {tag} vs composed", 1e-5)
    _compare(fused, ref, f"table {tag} vs float64", 1e-4)
    _compare(comp, ref, f"composed {tag} vs float64", 1e-4)
    again = _run_layer(name, d, masked, pb, True)
    assert torch.equal(again[0], fused[0])
    assert all(torch.equal(again[1][k], fused[1][k]) for k in NAMES)
    with torch.no_grad():                                # forward-only evaluation: null s and t
        q = _args(_operands(name, d, masked), False)
        args = [q[k] for k in NAMES] + [q["keep"]]
        o0, took = _took(lambda: Fn.GinLayerFn.apply(*args, pb))
        assert took == {"fused": 1, "composed": 0} and torch.equal(o0, fused[0])
        o1, took = _took(lambda: Fn.gin_layer(*args, pb))                 # ... and what gin_layer picks with the switch on
        assert took == {"fused": 1, "composed": 0} and torch.equal(o1, fused[0])


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
    from bmp._lib import ptr
    pb = to_dev(R.data("fixture")["pb"])
    assert pb.mt_row0 is None and not pb.oversized and pb.n_tiles >= 3
    N, nt = pb.n_rows, pb.n_tiles
    csr, csrT = (pb.csr_ptr, pb.csr_col, pb.csr_val), (pb.csrT_ptr, pb.csrT_col, pb.csrT_val)
    W = _weights(d, 40 + d)
    g = torch.Generator().manual_seed(41)
    h, dout = torch.randn(N, d, generator=g).to(dev()), torch.randn(N, d, generator=g).to(dev())
    keep = ((torch.rand(N, d, generator=g) >= P_DROP).float() * 2.0).to(dev()) if masked else None
    r0 = torch.arange(nt, dtype=torch.int32, device=dev()) * 128
    nb = torch.full((nt,), 4, dtype=torch.int32, device=dev())
    res = {}
    for entry, tab in (("tile", ()), ("table", (ptr(r0), ptr(nb), N, 0))):
        z = lambda: torch.zeros(N, d, device=dev())
        s, t, out, dp2, dp1, dh = z(), z(), z(), z(), z(), z()
        _abi_fwd(entry, d, nt, h, csr, W, keep, s, t, out, tab)
        _abi_bwd(entry, d, nt, dout, out, keep, t, csrT, W, dp2, dp1, dh, tab)
        torch.cuda.synchronize()
        res[entry] = dict(s=s, t=t, out=out, dp2=dp2, dp1=dp1, dh=dh)
    for k, x in res["table"].items():
        assert torch.isfinite(x).all(), k
        print(f"[whole tiles] d={d} masked={masked} {k}: max |table - tile| = {(x - res['tile'][k]).abs().max().item():.3e}")
        if (d, k) in CONTRACTED:
            close(x, res["tile"][k], f"table of whole tiles d={d}: {k}", tol=1e-5)
        else:
            assert torch.equal(x, res["tile"][k]), (k, (x - res["tile"][k]).abs().max().item())
    assert res["table"]["out"].abs().max() > 0 and res["table"]["dh"].abs().max() > 0


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "keep"])
def test_fixed_stride_clears_the_dead_rows(masked):
    """Through the C ABI at d = 64 on tiles of 1, 3 and 4 live blocks at stride 128: every output prefilled with NaN, the dead
    rows of h, keep, dout and (for the backward) out and t NaN too (never read), and a 128-row NaN canary behind mt_rows in every
    written array.  With tile_stride = 128 the rows of the dead blocks are exactly 0 in s, t, out, dp2, dp1 and dh and no NaN is
    left anywhere; the live rows equal the dense-row run (tile_stride = 0, which leaves the dead rows alone) of the same
    molecules; the canary stays NaN either way.  The forward with null s and t writes the same out."""
    from bmp._lib import ptr
    d, N, C = 64, 384, 128
    csr, csrT, r0, nb, live = _stride_case()
    W = _weights(d, 77)
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev())
    nan_dead = lambda x: torch.where(live[:, None], x, torch.full_like(x, float("nan")))
    h, dout = nan_dead(rnd(N, d)), nan_dead(rnd(N, d))
    keep = nan_dead(((torch.rand(N, d, generator=g) >= P_DROP).float() * 2.0).to(dev())) if masked else None
    nan = lambda: torch.full((N + C, d), float("nan"), device=dev())
    res = {}
    for stride in (128, 0):
        s, t, out, dp2, dp1, dh, out0 = nan(), nan(), nan(), nan(), nan(), nan(), nan()
        tab = (ptr(r0), ptr(nb), N, stride)
        _abi_fwd("table", d, 3, h, csr, W, keep, s, t, out, tab)
        _abi_fwd("table", d, 3, h, csr, W, keep, None, None, out0, tab)         # forward only: the same out, nothing else written
        torch.cuda.synchronize()
        assert torch.equal(out0[:N][live], out[:N][live]) and torch.isnan(out0[N:]).all()
        assert (out0[:N][~live] == 0).all() if stride else torch.isnan(out0[:N][~live]).all()
        res[stride] = dict(s=s, t=t.clone(), out=out.clone())
        out[:N] = nan_dead(out[:N]); t[:N] = nan_dead(t[:N])                     # the backward's inputs: dead rows NaN again
        _abi_bwd("table", d, 3, dout, out, keep, t, csrT, W, dp2, dp1, dh, tab)
        torch.cuda.synchronize()
        res[stride].update(dp2=dp2, dp1=dp1, dh=dh)
    for name, x in res[128].items():
        y = res[0][name]
        assert torch.isnan(x[N:]).all() and torch.isnan(y[N:]).all(), name       # the canary behind mt_rows
        x, y = x[:N], y[:N]
        assert not torch.isnan(x).any(), name
        assert (x[~live] == 0).all(), name
        assert torch.isfinite(x[live]).all(), name
        close(x[live], y[live], f"fixed stride masked={masked}: live rows of {name} vs dense rows", tol=1e-5)
        assert torch.isnan(y[~live]).all(), name          # (without a stride nothing is written there)
    assert res[128]["out"][:N][live].abs().max() > 0 and res[128]["dh"][:N][live].abs().max() > 0
    # a lone null of s / t is refused, as are a stride that is no multiple of 32 or shorter than a full tile and a missing table
    s, t, out, dp2, dp1, dh = (torch.empty(N, d, device=dev()) for _ in range(6))
    good = (ptr(r0), ptr(nb), N, 128)
    for s_, t_ in ((s, None), (None, t)):
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_fwd("table", d, 3, h, csr, W, keep, s_, t_, out, good)
    for tab in ((ptr(r0), ptr(nb), N, 96), (ptr(r0), ptr(nb), N, 130), (None, ptr(nb), N, 0), (ptr(r0), None, N, 0), (ptr(r0), ptr(nb), 0, 0)):
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_fwd("table", d, 3, h, csr, W, keep, s, t, out, tab)
        with pytest.raises(ValueError, match="argument check failed"):
            _abi_bwd("table", d, 3, dout, out, keep, t, csrT, W, dp2, dp1, dh, tab)


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
    pb, t, eb, t2 = _batches(dedup, n_cu)
    model = _pair_model(tied, attn)
    ran = 1 if tied else LAYERS
    assert model.training and model.graph_conv.rows_reason() is None and model.graph_conv.n_message_layers == ran
    inst, took = _took(lambda: _pair_run(model, pb, t))
    assert took == {"fused": ran, "composed": 0}, took
    at_inst = model.graph_conv.get_atom_array()
    enc, took = _took(lambda: _pair_run(model, eb, t2))
    assert took == {"fused": ran, "composed": 0}, took
    tag = f"gin tied={tied} attn={attn} dedup={dedup} n_cu={n_cu}"
    for k in ("y", "g1", "g2"):
        close(enc[k], inst[k], f"{tag}: {k} vs per-instance", tol=1e-5)
    loss_i, loss_e = model.loss(inst["y"], t).detach().reshape(1), model.loss(enc["y"], t2).detach().reshape(1)
    close(loss_e, loss_i, f"{tag}: loss vs per-instance", tol=1e-5)
    gmax = max(v.abs().max().item() for v in inst["grads"].values())
    assert sorted(enc["grads"]) == sorted(inst["grads"])
    for name, gr in enc["grads"].items():
        # (1e-3 of the largest gradient as the floor of a parameter's scale: test_gpu_ggate_enc.py)
        close(gr, inst["grads"][name], f"{tag}: grad {name} vs per-instance", tol=1e-5, floor=1e-3 * gmax)
    assert any(v.abs().max() > 0 for k, v in enc["grads"].items() if k.startswith("graph_conv/update_layers"))
    at_enc = model.graph_conv.get_atom_array()           # the atom array handed to the co-attention, on the instance rows
    assert at_enc.pb is eb.pb
    close(_atoms_by_molecule(at_enc.rows, eb.pb), _atoms_by_molecule(at_inst.rows, pb), f"{tag}: atoms", tol=1e-5)


def test_encode_rows_refuses_training_dropout_and_concat_of_several_layers(table_on):
    from bmp.ggnn import CONCAT_LAYOUT_REASON, DROPOUT_LAYOUT_REASON
    from bmp.predictor import build_pair_predictor
    pb, t, eb, t2 = _batches(True, 5)
    model = _pair_model(True, None, dropout_ratio=0.5)
    ev, took = _took(lambda: _pair_run(model.eval(), eb, t2, backward=False))        # evaluation mode: dropout is the identity
    assert took == {"fused": 1, "composed": 0} and torch.isfinite(ev["y"]).all()
    close(ev["y"], _pair_run(_pair_model(True, None).eval(), eb, t2, backward=False)["y"], "eval() ignores dropout_ratio", tol=1e-5)
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
    pb, t, eb, t2 = _batches(True, 5)
    model = _pair_model(False, None)
    res = {}
    for on in (True, False):
        monkeypatch.setitem(Fn.GIN_TABLE_DEFAULT, 64, on)
        res[on], took = _took(lambda: _pair_run(model, eb, t2))
        assert took == ({"fused": LAYERS, "composed": 0} if on else {"fused": 0, "composed": LAYERS}), (on, took)
    for k in ("y", "g1", "g2"):
        close(res[True][k], res[False][k], f"table kernels vs composed: {k}", tol=1e-5)
    gmax = max(v.abs().max().item() for v in res[False]["grads"].values())
    for name, gr in res[True]["grads"].items():
        close(gr, res[False]["grads"][name], f"table kernels vs composed: grad {name}", tol=1e-5, floor=1e-3 * gmax)


# ---- the fixed-shape batch ----
def _static_model(dropout_ratio=0.0):
    from bmp.gin import GIN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    torch.manual_seed(5)
    enc = GIN(out_dim=16, hidden_dim=64, n_layers=LAYERS, dropout_ratio=dropout_ratio, weight_tying=False)
    return GraphConvPredictorForPair(enc, None, build_link_predictor("hole", 16, 1)).to(dev())


@pytest.mark.parametrize("masked", [False, True], ids=["no-dropout", "given-masks"])
def test_static_batch_eager_step_equals_the_packed_step(masked, table_on):
    """Batch k0 holds the store's tallest molecules and batch k1, loaded into the same arrays afterwards, its shortest: rows that
    k0 left behind in a dead block would enter k1's weight gradients.  With masks: training mode at dropout_ratio = 0.5, the
    masks given, row for row the same in both layouts."""
    from bmp import packed
    from bmp.dp import FlatAdam
    ds, by_size, sizes = _static_world()
    B, d = 8, 64
    model = _static_model(P_DROP if masked else 0.0)
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
        if masked:
            r0p, r0s = pb.mol_row0.cpu().long(), sb.pb.mol_row0.cpu().long()
            nrows = pb.mol_nrows.cpu().long()
            assert torch.equal(nrows, sb.pb.mol_nrows.cpu().long())
            mp, msb = [], []
            for _ in range(LAYERS):
                k = (torch.rand(pb.n_rows, d, generator=g) >= P_DROP).float() / (1.0 - P_DROP)
                s = torch.ones(sb.pb.n_rows, d)
                for i in range(2 * B):
                    s[r0s[i]:r0s[i] + nrows[i]] = k[r0p[i]:r0p[i] + nrows[i]]
                mp.append(k.to(dev())); msb.append(s.to(dev()))
        model.graph_conv._dropout_masks = mp
        (loss, took) = _took(lambda: opt.functional_loss(pb, t=t))
        assert took == {"fused": LAYERS, "composed": 0}, took
        loss.backward(); opt.collect_grads()
        y_ref, g_ref, l_ref = model.y.detach().clone(), opt.grad.clone(), loss.detach().clone()
        model.graph_conv._dropout_masks = msb
        (loss, took) = _took(lambda: opt.functional_loss(sb.pb, t=sb.t))
        assert took == {"fused": LAYERS, "composed": 0}, took
        loss.backward(); opt.collect_grads()
        close(model.y.detach(), y_ref, f"static gin {tag}: logits", tol=1e-5)
        close(loss.detach().reshape(1), l_ref.reshape(1), f"static gin {tag}: loss", tol=1e-5)
        close(opt.grad, g_ref, f"static gin {tag}: flat gradient", tol=1e-5)
        assert g_ref.abs().max() > 0


def test_fit_runs_a_gin_model_in_every_layout(table_on):
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
        model = build_pair_predictor(encoder="gin", hidden_dim=64, out_dim=32, n_layers=2, attn="nie", head=4, dropout_ratio=0.0).to(dev())
        opt = FlatAdam(model, alpha=2e-3)
        tr = Tr.PairBatches(ds, i1[:144], i2[:144], lab[:144], 32, shuffle=True, seed=2, **kw)
        va = Tr.PairBatches(ds, i1[144:], i2[144:], lab[144:], 32, **kw)
        assert len(tr) == 5 and len(va) == 2
        tr.check_encoder(model)
        runs[name], took[name] = _took(lambda: Tr.fit(model, opt, tr, va, epochs=2))
        flat[name] = opt.flat.detach().clone()
    assert took["instance"]["composed"] == 0 and took["instance"]["fused"] > 0, took
    assert took["dedup"]["composed"] == 0 and took["dedup"]["fused"] > 0, took          # the table kernels, every step
    assert took["static"]["composed"] == 0 and 0 < took["static"]["fused"] < took["instance"]["fused"], took       # replays
    for name in ("dedup", "static"):
        for a, b in zip(runs["instance"], runs[name]):
            for key in ("main/loss", "validation/main/loss"):
                print(f"[fit] {name} {key}: {b[key]:.7f} vs per-instance {a[key]:.7f}")
        close(flat[name], flat["instance"], f"fit gin {name}: parameters after two passes vs per-instance", tol=1e-4)


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
        mark = dict(Fn.GIN_PATHS)
        lg.append(float(stepper(sb).detach()))
        assert Fn.GIN_PATHS["composed"] == mark["composed"]           # the recording took the table kernels, every call of it
        assert (Fn.GIN_PATHS["fused"] > mark["fused"]) == (k == 0)    # ... and a replay runs no Python step
    assert len(stepper.graphs) == 1 and og.t == oe.t == steps
    close(torch.tensor(lg), torch.tensor(le), f"recorded gin step: losses of {steps} steps", tol=1e-4)
    close(og.flat, oe.flat, f"recorded gin step: parameters after {steps} steps", tol=1e-4)
    assert not np.allclose(le[0], le[-1])
