"""GPU parity tests of the GIN encoder (bmp/gin.py, csrc/bmp_gin.hip) against the float64 dense restatement
(tests/gin_ref.py): g, get_atom_array().dense(side) and every parameter gradient at max-norm 1e-4 through parity_util.close.
Every case takes its (seed, shape, data) from gin_ref.KINK_TABLE (the relu kink condition, asserted on the CPU by
tests/test_gin_ref.py); the references are computed once per (row, options) and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gin_ref as GR                                  # noqa: E402
from oracle import ref_cpu as O                       # noqa: E402
from bmp import packed                                # noqa: E402
from test_gpu_ops import close, dev, to_dev, T        # noqa: E402

_REF = {}


def _ref(name, concat=False, activation="identity", real=None):
    """The restatement of a table row on every side of its data, differentiated once:
    dict(p (leaves with .grad), g, atoms [per side], cg, ca, keep (row masks or None))."""
    key = (name, concat, activation, real is not None)
    if key in _REF:
        return _REF[key]
    row = GR.KINK_TABLE[name]
    d = GR.data(row["data"])
    p = {k: v.requires_grad_() for k, v in GR.row_params(row, concat).items()}
    kr = GR.row_keep(row)
    outs = []
    for side, (atoms, adj) in enumerate(d["sides"]):
        kd = None if kr is None else GR.keep_dense(row["data"], kr, side)
        outs.append(GR.gin_forward(p, atoms, adj, row["tying"], concat, keep=kd, is_real_node=real, activation=activation))
    g = torch.cat([o[0] for o in outs])
    gen = torch.Generator().manual_seed(5)
    cg = torch.randn(g.shape, dtype=torch.float64, generator=gen)
    ca = [torch.randn(o[1].shape, dtype=torch.float64, generator=gen) for o in outs]
    ((g * cg).sum() + 0.1 * sum((o[1] * c).sum() for o, c in zip(outs, ca))).backward()
    _REF[key] = dict(p=p, g=g.detach(), atoms=[o[1].detach() for o in outs], cg=cg, ca=ca, keep=kr)
    return _REF[key]


def _enc(name, concat=False, activation="identity", dropout_ratio=0.0):
    from bmp.gin import GIN
    from bmp.snapshot import load_param_dict
    row = GR.KINK_TABLE[name]
    enc = GIN(out_dim=row["out"], hidden_dim=row["hidden"], n_layers=row["layers"], dropout_ratio=dropout_ratio,
              concat_hidden=concat, weight_tying=row["tying"], activation=activation).to(dev())
    load_param_dict(enc, GR.row_params(row, concat))
    return enc


def _run(enc, r, *args):
    """forward on ``args`` + the backward of the reference's scalar; returns (g, [dense atom states per side], grads)."""
    from bmp.snapshot import grad_dict
    g = enc(*args)
    at = enc.get_atom_array()
    dn = [at.dense(s) for s in range(len(r["ca"]))]
    d = dev()
    ((g * r["cg"].float().to(d)).sum() + 0.1 * sum((a * c.float().to(d)).sum() for a, c in zip(dn, r["ca"]))).backward()
    return g.detach(), [a.detach() for a in dn], grad_dict(enc)


def _check(res, r, tag=""):
    g, dn, gd = res
    close(g, r["g"], tag + "g")
    for s, a in enumerate(dn):
        close(a, r["atoms"][s], f"{tag}atoms {s + 1}")
    assert sorted(gd) == sorted(r["p"])
    for k, gr in gd.items():         # (a readout layer the tied loop never reaches has no gradient on either side: zero)
        want = r["p"][k].grad
        close(gr, want if want is not None else torch.zeros_like(r["p"][k]), f"{tag}grad {k}")


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.GIN_PATHS)
    out = fn()
    return out, {k: Fn.GIN_PATHS[k] - before[k] for k in before}


def _pb(name):
    return to_dev(GR.data(GR.KINK_TABLE[name]["data"])["pb"])


def test_fixture_tied_default_with_tanh_readout():
    """The trainer's shape of model -- tied, n_layers = 4, so ONE layer runs -- on the 40-molecule store, 13 + 13 instances, with the
    readout's activation given as a string."""
    r = _ref("c24", activation="tanh")
    enc = _enc("c24", activation="tanh")
    assert enc.n_message_layers == 1 and enc.n_layers == 4
    res, took = _took(lambda: _run(enc, r, _pb("c24")))
    assert took == {"fused": 0, "composed": 1}, took
    _check(res, r)


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("name,path,steps", [("c16", "composed", 2), ("c24", "composed", 1), ("f64", "fused", 3), ("f128", "fused", 2)])
def test_gin_matches_dense_restatement(name, path, steps, concat):
    r = _ref(name, concat)
    enc = _enc(name, concat)
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took == {path: steps, ("composed" if path == "fused" else "fused"): 0}, took
    row = GR.KINK_TABLE[name]
    assert res[0].shape == (26, (steps if concat else 1) * row["out"])
    _check(res, r)


@pytest.mark.parametrize("name", ["f64", "f128"])
def test_fused_and_composed_paths_agree(name, monkeypatch):
    """The fused tile kernels against the existing operators (message operator with W1 for every bond type + row linear), forced
    through the layer's private switch, on the same inputs: both float32, different summation orders.  The two runs must
    really take the two paths."""
    from bmp.gin import GINUpdate
    r = _ref(name)
    steps = GR.KINK_TABLE[name]["layers"]
    res = []
    for fused in (True, False):
        monkeypatch.setattr(GINUpdate, "_fused", fused)
        out, took = _took(lambda: _run(_enc(name), r, _pb(name)))
        assert took == ({"fused": steps, "composed": 0} if fused else {"fused": 0, "composed": steps}), took
        res.append(out)
    close(res[0][0], res[1][0], "fused vs composed g")
    for s in range(2):
        close(res[0][1][s], res[1][1][s], f"fused vs composed atoms {s + 1}")
    for k in res[0][2]:
        close(res[0][2][k], res[1][2][k], f"fused vs composed grad {k}")
    assert not torch.equal(res[0][1][0], res[1][1][0])


@pytest.mark.parametrize("name", ["over16", "over64"])
def test_molecule_spanning_tiles_takes_the_composed_path(name):
    """One molecule of 150 atoms: its bonds cross the tile boundary, so the tile-local kernels must not run, at a width
    they support (64) as at one they do not (16)."""
    pb = _pb(name)
    assert pb.oversized and pb.max_rows_per_mol == 151
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name), r, pb))
    assert took == {"fused": 0, "composed": 2}, took
    _check(res, r)


@pytest.mark.parametrize("name", ["small16", "small64"])
def test_dense_call_form_equals_packed_form(name):
    atoms, adj = GR.data("small")["sides"][0]
    r = _ref(name)
    pb = packed.pack_from_dense([atoms], [adj], device=dev())
    a = _run(_enc(name), r, pb)
    b = _run(_enc(name), r, atoms, adj)
    for other in (b,):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1][0], other[1][0])
        for k in a[2]:
            assert torch.equal(a[2][k], other[2][k]), k
    _check(a, r)


def test_is_real_node_matches_restatement():
    atoms, adj = GR.data("small")["sides"][0]
    real = (np.random.RandomState(3).uniform(size=atoms.shape) < 0.7).astype(np.float32)
    assert real[atoms == 0].any() and not real.all()                    # padded positions counted, real atoms dropped
    r = _ref("small16", real=real)
    _check(_run(_enc("small16"), r, atoms, adj, real), r)


@pytest.mark.parametrize("name,path", [("keep16", "composed"), ("keep64", "fused")])
def test_training_mode_with_a_given_keep_mask(name, path):
    r = _ref(name)
    enc = _enc(name, dropout_ratio=GR.KINK_TABLE[name]["drop"][0])
    enc._dropout_masks = [k.to(dev()) for k in r["keep"]]
    assert enc.training
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took[path] == 2 and sum(took.values()) == 2, took
    _check(res, r)
    assert (res[1][0] == 0).float().mean() > 0.4                        # the mask bit: at least the dropped half is zero


@pytest.mark.parametrize("name", ["c16", "f64"])
def test_eval_ignores_dropout_ratio(name):
    r = _ref(name)
    pb = _pb(name)
    plain = _run(_enc(name, dropout_ratio=0.0), r, pb)
    enc = _enc(name, dropout_ratio=0.5).eval()
    enc._dropout_masks = [torch.zeros(pb.n_rows, GR.KINK_TABLE[name]["hidden"], device=dev())] * 3      # must not be read
    ev = _run(enc, r, pb)
    assert torch.equal(ev[0], plain[0]) and torch.equal(ev[1][0], plain[1][0])
    _check(ev, r)
    enc = _enc(name, dropout_ratio=0.5)                                 # training: a mask is drawn
    with torch.no_grad():
        enc(pb)
    h = enc.get_atom_array().dense(0)
    assert (h == 0).float().mean() > (ev[1][0] == 0).float().mean() + 0.1


def test_pair_model_one_training_step():
    """GIN + Nie co-attention + MLP as build_pair_predictor builds it for the trainer (tied, concat_hidden, dropout 0.5, training
    mode, the masks given): loss, logits and every gradient of one eager FlatAdam step against the restatement's."""
    from bmp.dp import FlatAdam
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    row = GR.KINK_TABLE["pair16"]
    d = GR.data(row["data"])
    hidden, out = row["hidden"], row["out"]
    lab = np.random.RandomState(4).randint(0, 2, (13, 1)).astype(np.int32)
    dr = O._Draw(21, torch.float64, 0.1)
    O.init_nie(dr, "attn/", hidden, out, 8)
    O.init_mlp(dr, "mlp/", 2 * out, 1, (32, 16))
    p = dict(dr.p)
    p.update(GR.row_params(row, True, prefix="graph_conv/"))
    q = {k: v.clone().requires_grad_() for k, v in p.items()}
    kr = GR.row_keep(row)
    at = [GR.gin_forward(q, *d["sides"][s], True, True, keep=GR.keep_dense(row["data"], kr, s), prefix="graph_conv/")[1] for s in (0, 1)]
    g1, g2 = O.nie_coattention(q, at[0], at[1], "tanh", prefix="attn/")
    y_o = O.mlp_forward(q, torch.cat((g1, g2), dim=-1), 2)
    loss_o = O.sigmoid_cross_entropy(y_o, T(lab))
    names = sorted(q)
    gr = torch.autograd.grad(loss_o, [q[n] for n in names], allow_unused=True)
    g_o = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, gr)}      # (the readout feeds nobody here)
    model = build_pair_predictor(hidden_dim=hidden, out_dim=out, n_layers=row["layers"], attn="nie", encoder="gin").to(dev())
    load_param_dict(model, p)
    model.graph_conv._dropout_masks = [k.to(dev()) for k in kr]
    assert model.training and model.graph_conv.dropout_ratio == 0.5
    opt = FlatAdam(model, alpha=1e-2)
    y = opt.functional_forward(_pb("pair16"))
    loss = model.loss(y, T(lab).to(dev()))
    loss.backward()
    opt.collect_grads()
    close(y, y_o, "logits"); close(loss, loss_o, "loss")
    off = 0
    for name, shp in zip(opt.names, opt.shapes):
        n = int(np.prod(shp))
        close(opt.grad[off:off + n].view(shp), g_o[name.replace(".", "/")], f"grad {name}")
        off += n
    before = opt.flat.clone()
    opt.step()
    assert torch.isfinite(opt.flat).all() and not torch.equal(opt.flat, before)
