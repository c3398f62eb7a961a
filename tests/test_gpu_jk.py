"""GPU parity tests of the jumping-knowledge GGNN encoders (bmp/ggnn_jk.py on the kernels of csrc/bmp_jk.hip) against the float64
dense restatement (tests/jk_ref.py): g, get_atom_array().dense(side) and every parameter gradient at max-norm 1e-4 through
parity_util.close.  Every case takes its (kind, seed, shape, data) from jk_ref.CASES; the references are computed once per
(case, options) and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggate32_ref as G32                             # noqa: E402
import jk_ref as R                                    # noqa: E402
from bmp import packed                                # noqa: E402
from test_gpu_ops import close, dev, to_dev, T        # noqa: E402

_REF = {}


def _ref(name, concat=False, keep_seed=None):
    key = (name, concat, keep_seed)
    if key not in _REF:
        _REF[key] = R.reference(name, concat, keep_seed)
    return _REF[key]


def _enc(name, concat=False, fused=True, dropout=0.0):
    from bmp.ggnn_jk import JKGruGGNN, JKNetGGNN
    from bmp.snapshot import load_param_dict
    c = R.CASES[name]
    kw = dict(out_dim=c["out"], hidden_dim=c["hidden"], n_layers=c["layers"], concat_hidden=concat, weight_tying=c["tying"],
              update_tying=c["update_tying"], dropout_rate=dropout)
    enc = (JKNetGGNN(layer_aggr=c["aggr"], **kw) if c["kind"] == "jknet" else JKGruGGNN(self_loop=c["loop"], **kw)).to(dev())
    load_param_dict(enc, R.case_params(c, concat))
    enc._fused = fused
    return enc


def _run(enc, r, *args):
    """forward on ``args`` + the backward of the reference's scalar; returns (g, [dense atom states per side], grads)."""
    from bmp.snapshot import grad_dict
    g = enc(*args)
    at = enc.get_atom_array()
    dn = [at.dense(s) for s in range(len(r["ca"]))]
    d = dev()
    ((g * r["cg"].float().to(d)).sum() + 0.1 * sum((a * w.float().to(d)).sum() for a, w in zip(dn, r["ca"]))).backward()
    return g.detach(), [a.detach() for a in dn], grad_dict(enc)


def _check(res, r, tag=""):
    g, dn, gd = res
    close(g, r["g"], tag + "g")
    for s, a in enumerate(dn):
        close(a, r["atoms"][s], f"{tag}atoms {s + 1}")
    assert sorted(gd) == sorted(r["p"])
    for k, gr in gd.items():         # (a link that is never called has no gradient on either side: zero)
        want = r["p"][k].grad
        close(gr, want if want is not None else torch.zeros_like(r["p"][k]), f"{tag}grad {k}")


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.JK_PATHS)
    out = fn()
    return out, {k: Fn.JK_PATHS[k] - before[k] for k in before}


def _pb(name):
    return to_dev(R.data(R.CASES[name]["data"])["pb"])


@pytest.fixture
def fused_on(monkeypatch):
    """Every (kind, width) on the fused kernels, whatever the dispatch table says: the kernels are tested either way."""
    from bmp import functional as Fn
    monkeypatch.setattr(Fn, "JK_STEP_DEFAULT", {k: True for k in Fn.JK_STEP_DEFAULT})


FUSED = ["max64", "mean64", "attn64", "attn64u", "attn128", "concat64", "gru64", "gru64u", "gru128", "gru64t", "attn_blocks64",
         "gru_blocks64", "max_dense64", "gru_dense64"]
COMPOSED = ["attn16", "mean24", "gru32", "attn_over64", "gru_over64"]


@pytest.mark.parametrize("name", FUSED + COMPOSED)
def test_matches_dense_restatement(name, fused_on):
    c = R.CASES[name]
    pb = _pb(name)
    if c["data"] == "blocks":
        assert G32.blocks_property(R.data("blocks")["pb"])
    if c["data"] == "dense":         # more CSR entries than fit a staging buffer: both directions gather from global memory
        assert G32.dense_property(R.data("dense")["pb"])
    if c["data"] == "oversized":     # one molecule of 150 atoms: its bonds cross the tile boundary, the tile-local kernels must not run
        assert pb.oversized and pb.max_rows_per_mol == 151
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, pb))
    want = "fused" if name in FUSED else "composed"
    assert took == {want: c["layers"], "fused" if want == "composed" else "composed": 0}, took
    assert res[0].shape == (R.data(c["data"])["pb"].n_mols, c["out"])
    _check(res, r)
    if name == "gru64t":             # update layer 1 is built and never read
        assert res[2]["update_layers_0/1/W"].abs().max() == 0 and res[2]["update_layers_0/0/W"].abs().max() > 0
    if c["kind"] == "jk_gru" and c["layers"] > 1:
        assert res[2]["update_layer/U/W"].abs().max() > 0
    if c["aggr"] == "attn":          # the coefficients themselves, per batch side
        from bmp import functional as Fn
        co = Fn.JKAggFn.last_coef
        assert co.shape == (len(r["coef"]), c["layers"])
        for s, want_c in enumerate(r["coef"]):
            close(co[s], want_c, f"coef side {s + 1}")


@pytest.mark.parametrize("name", ["attn64", "gru64", "mean24"])
def test_concat_hidden(name, fused_on):
    c = R.CASES[name]
    r = _ref(name, concat=True)
    res = _run(_enc(name, concat=True).eval(), r, _pb(name))
    assert res[0].shape == (R.data(c["data"])["pb"].n_mols, c["layers"] * c["out"])
    _check(res, r)


@pytest.mark.parametrize("name", ["attn64", "gru128"])
def test_dispatch_follows_the_measured_table(name):
    """Without the override: Fn.jk_step sends a (kind, width) to the fused kernels iff JK_STEP_DEFAULT says so."""
    from bmp import functional as Fn
    c = R.CASES[name]
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, _pb(name)))
    path = "fused" if Fn.JK_STEP_DEFAULT[(c["kind"], c["hidden"])] else "composed"
    assert took == {path: c["layers"], "composed" if path == "fused" else "fused": 0}, took
    _check(res, r)


@pytest.mark.parametrize("name", ["attn64u", "attn128", "gru64", "gru128", "gru_blocks64", "max_dense64"])
def test_fused_and_composed_paths_agree(name, fused_on):
    """The fused kernels against the existing operators (message operator + row linear with relu), forced through the encoder's
    private switch, on the same inputs: both float32, different summation orders.  The two runs must really take the two paths."""
    r = _ref(name)
    steps = R.CASES[name]["layers"]
    res = []
    for fused in (True, False):
        out, took = _took(lambda: _run(_enc(name, fused=fused).eval(), r, _pb(name)))
        assert took == ({"fused": steps, "composed": 0} if fused else {"fused": 0, "composed": steps}), took
        res.append(out)
    close(res[0][0], res[1][0], "fused vs composed g")
    for s in range(len(res[0][1])):
        close(res[0][1][s], res[1][1][s], f"fused vs composed atoms {s + 1}")
    for k in res[0][2]:
        close(res[0][2][k], res[1][2][k], f"fused vs composed grad {k}")
    # (no `not torch.equal` here: both forms run exact-f32 MFMAs over k in the same order and relu rounds nothing, so the atom
    # states may agree bit for bit; that the two paths were taken is what JK_PATHS showed above)


@pytest.mark.parametrize("name", ["attn_drop64", "gru_drop64"])
def test_training_dropout_with_given_masks_takes_the_composed_path(name, fused_on):
    """Training mode with the masks given (ratio 0.25: 1 / 0.75 or 0): the aggregator sees the dropped states, jk_gru's GRU keeps
    its own un-dropped state; evaluation mode does not read the masks and runs fused."""
    c = R.CASES[name]
    r = _ref(name, keep_seed=R.KEEP_SEEDS[name])
    pb = _pb(name)
    enc = _enc(name, dropout=R.DROP_P)
    enc._dropout_masks = [k.to(dev()) for k in r["keep"]]
    assert enc.training
    res, took = _took(lambda: _run(enc, r, pb))
    assert took == {"fused": 0, "composed": c["layers"]}, took
    _check(res, r)
    plain = _ref(name)
    ev = _enc(name, dropout=R.DROP_P).eval()
    ev._dropout_masks = [torch.zeros(pb.n_rows, c["hidden"], device=dev())] * c["layers"]       # must not be read
    out, took = _took(lambda: _run(ev, plain, pb))
    assert took == {"fused": c["layers"], "composed": 0}, took
    _check(out, plain, "eval ")
    assert not torch.equal(out[1][0], res[1][0])


@pytest.mark.parametrize("name", ["attn_small64", "gru_small64"])
def test_dense_call_form_equals_packed_form(name, fused_on):
    atoms, adj = R.data("small")["sides"][0]
    r = _ref(name)
    pb = packed.pack_from_dense([atoms], [adj], device=dev())
    a, took = _took(lambda: _run(_enc(name).eval(), r, pb))
    assert took == {"fused": 2, "composed": 0}, took
    b = _run(_enc(name).eval(), r, atoms, adj)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    _check(a, r)


@pytest.mark.parametrize("name", ["attn64", "gru64"])
def test_forward_only_form_is_bit_identical(name, fused_on):
    """Under torch.no_grad() the step passes a null m (the instance that saves nothing): the same values, bit for bit."""
    pb = _pb(name)
    enc = _enc(name).eval()
    g = enc(pb)
    h = enc.get_atom_array().dense(0)
    with torch.no_grad():
        (g0, took) = _took(lambda: enc(pb))
        h0 = enc.get_atom_array().dense(0)
    assert took == {"fused": R.CASES[name]["layers"], "composed": 0}, took
    assert g.requires_grad and not g0.requires_grad
    assert torch.equal(g.detach(), g0) and torch.equal(h.detach(), h0)


@pytest.mark.parametrize("name", ["attn64", "attn_drop64"])
def test_two_runs_give_bit_identical_results(name, fused_on):
    ks = R.KEEP_SEEDS.get(name)
    r = _ref(name, keep_seed=ks)
    res = []
    for _ in range(2):
        enc = _enc(name, dropout=R.DROP_P if ks else 0.0)
        if ks is not None:
            enc._dropout_masks = [k.to(dev()) for k in r["keep"]]
        else:
            enc.eval()
        res.append(_run(enc, r, _pb(name)))
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


def test_mean_and_attn_aggregators_alone():
    """Fn.JKAggFn on random row tensors over a two-sided batch against float64: y, the coefficients and every dH_t, with the row
    weights (pad rows of multiplicity > 1, fill rows of weight 0) and the per-side sums by hand."""
    from bmp import functional as Fn
    pb = _pb("attn64")
    assert len(pb.side_tiles) == 3 and pb.side_tiles[1] < pb.n_tiles
    gen = torch.Generator().manual_seed(3)
    for T_, d in ((1, 8), (3, 20), (8, 64)):
        hs64 = [(0.01 * torch.randn(pb.n_rows, d, dtype=torch.float64, generator=gen)).requires_grad_() for _ in range(T_)]
        dy = torch.randn(pb.n_rows, d, dtype=torch.float64, generator=gen)
        w = pb.row_w.double().cpu()
        side = (torch.arange(pb.n_rows) >= pb.side_tiles[1] * 128).long()
        for mode in ("mean", "attn"):
            if mode == "mean":
                coef = torch.full((2, T_), 1.0 / T_, dtype=torch.float64)
            else:
                E = torch.stack([torch.stack([(w[side == s, None] * hs64[t][side == s] * (hs64[-1][side == s] + hs64[0][side == s])).sum()
                                              for t in range(T_)]) for s in (0, 1)])
                coef = torch.softmax(E, dim=1)
            y64 = sum(coef[side, t][:, None] * hs64[t] for t in range(T_))
            g64 = torch.autograd.grad((y64 * dy).sum(), hs64)
            hs = [h.detach().float().to(dev()).requires_grad_() for h in hs64]
            y = Fn.JKAggFn.apply(Fn.JK_AGG_MODE[mode], pb, *hs)
            close(Fn.JKAggFn.last_coef, coef, f"{mode} T={T_} coef")
            close(y, y64, f"{mode} T={T_} y")
            gr = torch.autograd.grad((y * dy.float().to(dev())).sum(), hs)
            for t in range(T_):
                close(gr[t], g64[t], f"{mode} T={T_} dH_{t + 1}")


def test_jk_step_fn_refuses_other_widths_and_the_entries_bad_arguments():
    from bmp import _lib, functional as Fn
    from bmp._lib import check, ptr, stream
    pb = _pb("attn16")
    z = lambda *s: torch.zeros(*s, device=dev())
    with pytest.raises(ValueError, match=r"\{64, 128\}"):
        Fn.JKStepFn.apply(z(pb.n_rows, 16), z(64, 16), z(4, 16), None, None, z(32, 16), z(16), pb)
    d = 64
    out = z(128, d) + 7.0
    cp = torch.zeros(129, dtype=torch.int32, device=dev())
    a = dict(h=z(128, d), W=z(4 * d, d), bE=z(4, d), AU=z(2 * d, d), bU=z(d), m=z(128, d), ws=z(d, d))
    L = _lib.lib()
    for bad in (dict(ng=3), dict(off=4), dict(bs=False)):    # a third width, a pointer 4 bytes off, a self loop without its bias
        with pytest.raises(ValueError, match="bmp_jk_step_tile_fwd: argument check failed"):
            check(L.bmp_jk_step_tile_fwd(bad.get("ng", 1), ptr(a["h"]) + bad.get("off", 0), 1, d, ptr(cp), ptr(cp), ptr(a["bU"]),
                                         ptr(a["W"]), ptr(a["bE"]), ptr(a["ws"]) if "bs" in bad else None, None, ptr(a["AU"]),
                                         ptr(a["bU"]), ptr(a["m"]), ptr(out), stream()), "bmp_jk_step_tile_fwd")
    torch.cuda.synchronize()
    assert (out == 7.0).all()


@pytest.mark.parametrize("name", ["attn_pair64", "gru_pair64"])
def test_pair_model_one_training_step(name, fused_on):
    """One eager FlatAdam step of GraphConvPredictorForPair with each new encoder (no co-attention, MLP link predictor), in
    training mode with the dropout masks given: loss, logits and the whole flat gradient against the restatement."""
    from bmp.dp import FlatAdam
    from bmp.predictor import GraphConvPredictorForPair
    from bmp.mlp import MLP
    from bmp.snapshot import load_param_dict
    c = R.CASES[name]
    ref = R.pair_reference(name)
    from bmp.ggnn_jk import JKGruGGNN, JKNetGGNN
    kw = dict(out_dim=c["out"], hidden_dim=c["hidden"], n_layers=c["layers"], weight_tying=c["tying"], update_tying=c["update_tying"],
              dropout_rate=R.DROP_P)
    enc = JKNetGGNN(layer_aggr=c["aggr"], **kw) if c["kind"] == "jknet" else JKGruGGNN(self_loop=c["loop"], **kw)
    model = GraphConvPredictorForPair(enc, None, MLP(1, R.PAIR_HIDDEN_DIMS, in_dim=2 * c["out"])).to(dev())
    load_param_dict(model, R.pair_params(name))
    model.graph_conv._dropout_masks = [k.to(dev()) for k in ref["keep"]]
    assert model.training
    opt = FlatAdam(model, alpha=1e-2)
    lab = T(R.pair_labels()).to(dev())
    (y, took) = _took(lambda: opt.functional_forward(_pb(name)))
    assert took == {"fused": 0, "composed": c["layers"]}, took           # training dropout
    loss = model.loss(y, lab)
    loss.backward()
    opt.collect_grads()
    close(y, ref["y"], "logits"); close(loss, ref["loss"], "loss")
    off, seen = 0, set()
    for pname, shp in zip(opt.names, opt.shapes):
        n = int(np.prod(shp))
        key = pname.replace(".", "/")
        close(opt.grad[off:off + n].view(shp), ref["grads"][key], f"grad {pname}")
        seen.add(key)
        off += n
    assert seen == set(ref["grads"])
    before = opt.flat.clone()
    opt.step()
    assert torch.isfinite(opt.flat).all() and not torch.equal(opt.flat, before)


def test_attn_encoder_is_refused_by_the_encoder_layout_and_dedup():
    from bmp.ggnn_jk import JK_ATTN_LAYOUT_REASON
    from bmp.predictor import build_pair_predictor
    from bmp.trainer import PairBatches
    model = build_pair_predictor(hidden_dim=64, out_dim=16, n_layers=2, attn=None, encoder="ggnn-jknet").to(dev())
    idx, lab = np.arange(3), np.zeros((3, 1), np.int32)
    for kw in (dict(layout="encoder"), dict(layout="encoder", dedup=True)):
        with pytest.raises(NotImplementedError) as e:
            PairBatches(None, idx, idx, lab, 2, **kw).check_encoder(model)
        assert JK_ATTN_LAYOUT_REASON in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        model.graph_conv.encode_rows(_pb("attn64"))
    assert JK_ATTN_LAYOUT_REASON in str(e.value)
