"""GPU parity tests of the fuse-gate and simple-gate GGNN encoders (bmp/ggnn_gate.py, csrc/bmp_gate.hip) against the float64
dense restatement (tests/ggate_ref.py): g, get_atom_array().dense(side) and every parameter gradient at max-norm 1e-4 through
parity_util.close.  Every case takes its (kind, seed, shape, data) from ggate_ref.CASES; the references are computed once per
(case, options) and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggate_ref as R                                 # noqa: E402
from oracle import ref_cpu as O                       # noqa: E402
from bmp import packed                                # noqa: E402
from test_gpu_ops import close, dev, to_dev, T        # noqa: E402

_REF = {}


def _ref(name, concat=False, keep_seed=None):
    """The restatement of a case on every side of its data, differentiated once:
    dict(p (leaves with .grad), g, atoms [per side], cg, ca, keep (row masks or None))."""
    key = (name, concat, keep_seed)
    if key in _REF:
        return _REF[key]
    c = R.CASES[name]
    d = R.data(c["data"])
    p = {k: v.requires_grad_() for k, v in R.case_params(c, concat).items()}
    kr = None if keep_seed is None else R.keep_rows(c["data"], c["hidden"], c["layers"], keep_seed)
    outs = []
    for side, (atoms, adj) in enumerate(d["sides"]):
        kd = None if kr is None else R.keep_dense(c["data"], kr, side)
        outs.append(R.case_forward(c, p, atoms, adj, concat, keep=kd))
    g = torch.cat([o[0] for o in outs])
    gen = torch.Generator().manual_seed(5)
    cg = torch.randn(g.shape, dtype=torch.float64, generator=gen)
    ca = [torch.randn(o[1].shape, dtype=torch.float64, generator=gen) for o in outs]
    ((g * cg).sum() + 0.1 * sum((o[1] * w).sum() for o, w in zip(outs, ca))).backward()
    _REF[key] = dict(p=p, g=g.detach(), atoms=[o[1].detach() for o in outs], cg=cg, ca=ca, keep=kr)
    return _REF[key]


def _enc(name, concat=False, fused=True):
    from bmp.ggnn_gate import FuseGGNN, GateGGNN
    from bmp.snapshot import load_param_dict
    c = R.CASES[name]
    kw = dict(out_dim=c["out"], hidden_dim=c["hidden"], n_layers=c["layers"], concat_hidden=concat, weight_tying=c["tying"])
    enc = (FuseGGNN(**kw) if c["kind"] == "fuse" else GateGGNN(update_tying=c["update_tying"], **kw)).to(dev())
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
    for k, gr in gd.items():         # (a link the file constructs and never calls has no gradient on either side: zero)
        want = r["p"][k].grad
        close(gr, want if want is not None else torch.zeros_like(r["p"][k]), f"{tag}grad {k}")


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.GATE_PATHS)
    out = fn()
    return out, {k: Fn.GATE_PATHS[k] - before[k] for k in before}


def _pb(name):
    return to_dev(R.data(R.CASES[name]["data"])["pb"])


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("name,path", [("fuse16", "composed"), ("fuse24", "composed"), ("fuse64", "fused"), ("fuse128", "fused"),
                                       ("gate16", "composed"), ("gate24", "composed"), ("gate64", "fused"), ("gate128", "fused")])
def test_matches_dense_restatement(name, path, concat):
    c = R.CASES[name]
    r = _ref(name, concat)
    enc = _enc(name, concat).eval()
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took == {path: c["layers"], ("composed" if path == "fused" else "fused"): 0}, took
    assert res[0].shape == (26, (c["layers"] if concat else 1) * c["out"])
    _check(res, r)
    if c["kind"] == "fuse":          # the links nobody calls get no gradient
        assert all(v.abs().max() == 0 for k, v in res[2].items() if k.startswith("update_layer/") or k.startswith("embed_linear/"))


@pytest.mark.parametrize("name", ["fuse64", "fuse128", "gate64", "gate128"])
def test_fused_and_composed_paths_agree(name):
    """The fused tile kernels against the existing operators (message operator + row linear + torch elementwise), forced through
    the encoder's private switch, on the same inputs: both float32, different summation orders.  The two runs must really take
    the two paths."""
    r = _ref(name)
    steps = R.CASES[name]["layers"]
    res = []
    for fused in (True, False):
        out, took = _took(lambda: _run(_enc(name, fused=fused).eval(), r, _pb(name)))
        assert took == ({"fused": steps, "composed": 0} if fused else {"fused": 0, "composed": steps}), took
        res.append(out)
    close(res[0][0], res[1][0], "fused vs composed g")
    for s in range(2):
        close(res[0][1][s], res[1][1][s], f"fused vs composed atoms {s + 1}")
    for k in res[0][2]:
        close(res[0][2][k], res[1][2][k], f"fused vs composed grad {k}")
    assert not torch.equal(res[0][1][0], res[1][1][0])


@pytest.mark.parametrize("name", ["fuse_over16", "fuse_over64", "gate_over16", "gate_over64"])
def test_molecule_spanning_tiles_takes_the_composed_path(name):
    """One molecule of 150 atoms: its bonds cross the tile boundary, so the tile-local kernels must not run, at a width
    they support (64) as at one they do not (16)."""
    pb = _pb(name)
    assert pb.oversized and pb.max_rows_per_mol == 151
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, pb))
    assert took == {"fused": 0, "composed": 2}, took
    _check(res, r)


@pytest.mark.parametrize("name", ["fuse_small16", "gate_small64"])
def test_dense_call_form_equals_packed_form(name):
    atoms, adj = R.data("small")["sides"][0]
    r = _ref(name)
    pb = packed.pack_from_dense([atoms], [adj], device=dev())
    a = _run(_enc(name).eval(), r, pb)
    b = _run(_enc(name).eval(), r, atoms, adj)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    _check(a, r)


@pytest.mark.parametrize("name,path", [("fuse_keep16", "composed"), ("fuse_keep64", "fused")])
def test_fuse_training_mode_with_given_masks(name, path):
    """Training mode: the fuse gate's dropout on r * h with the masks given (ratio 0.05: 1 / 0.95 or 0); evaluation mode does not
    read them."""
    r = _ref(name, keep_seed=11)
    pb = _pb(name)
    enc = _enc(name)
    enc._dropout_masks = [k.to(dev()) for k in r["keep"]]
    assert enc.training
    res, took = _took(lambda: _run(enc, r, pb))
    assert took[path] == 2 and sum(took.values()) == 2, took
    _check(res, r)
    plain = _ref(name)
    ev = _enc(name).eval()
    ev._dropout_masks = [torch.zeros(pb.n_rows, R.CASES[name]["hidden"], device=dev())] * 2       # must not be read
    out = _run(ev, plain, pb)
    _check(out, plain, "eval ")
    assert not torch.equal(out[1][0], res[1][0])
    drawn = _enc(name)                                                  # training without given masks: one is drawn per step
    with torch.no_grad():
        drawn(pb)
    assert not torch.equal(drawn.get_atom_array().dense(0), out[1][0])


@pytest.mark.parametrize("name,path", [("gate16u", "composed"), ("gate64u", "fused")])
def test_gate_with_untied_update_layers(name, path):
    r = _ref(name)
    enc = _enc(name)
    assert len(enc.gate_layer) == 3 and not enc.update_tying
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took[path] == 3 and sum(took.values()) == 3, took
    _check(res, r)
    assert all(res[2][f"gate_layer/{k}/W"].abs().max() > 0 for k in range(3))


def test_pair_model_one_training_step():
    """Fuse-gate GGNN + Nie co-attention + MLP as build_pair_predictor builds it (tied, training mode, the masks given): loss,
    logits and every gradient of one eager FlatAdam step against the restatement's."""
    from bmp.dp import FlatAdam
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    c = R.CASES["fuse_pair16"]
    d = R.data(c["data"])
    hidden, out = c["hidden"], c["out"]
    lab = np.random.RandomState(4).randint(0, 2, (13, 1)).astype(np.int32)
    dr = O._Draw(21, torch.float64, 0.1)
    O.init_nie(dr, "attn/", hidden, out, 8)
    O.init_mlp(dr, "mlp/", 2 * out, 1, (32, 16))
    p = dict(dr.p)
    p.update(R.case_params(c, prefix="graph_conv/"))
    q = {k: v.clone().requires_grad_() for k, v in p.items()}
    kr = R.keep_rows(c["data"], hidden, c["layers"], 13)
    at = [R.case_forward(c, q, *d["sides"][s], keep=R.keep_dense(c["data"], kr, s), prefix="graph_conv/")[1] for s in (0, 1)]
    g1, g2 = O.nie_coattention(q, at[0], at[1], "tanh", prefix="attn/")
    y_o = O.mlp_forward(q, torch.cat((g1, g2), dim=-1), 2)
    loss_o = O.sigmoid_cross_entropy(y_o, T(lab))
    names = sorted(q)
    gr = torch.autograd.grad(loss_o, [q[n] for n in names], allow_unused=True)
    g_o = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, gr)}      # (the readout feeds nobody here)
    model = build_pair_predictor(hidden_dim=hidden, out_dim=out, n_layers=c["layers"], attn="nie", encoder="ggnn-fuse").to(dev())
    load_param_dict(model, p)
    model.graph_conv._dropout_masks = [k.to(dev()) for k in kr]
    assert model.training
    opt = FlatAdam(model, alpha=1e-2)
    y = opt.functional_forward(_pb("fuse_pair16"))
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
