"""GPU parity tests of the ggnn_dev and self-loop GGNN encoders (bmp/ggnn_dev.py, csrc/bmp_loop.hip) against the float64 dense
restatement (tests/ggdev_ref.py): molecule vectors, atom arrays and every parameter gradient at max-norm 1e-4 through
parity_util.close (the float32 restatement lies within 1.7e-6 of the float64 one on these shapes, forward and gradients: the
bound is about 60 times the arithmetic's own error).  Every case takes its (kind, seed, shape, data) from ggdev_ref.CASES; the
references are computed once per (case, options) and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggdev_ref as R                                 # noqa: E402
from oracle import ref_cpu as O                       # noqa: E402
from bmp import packed                                # noqa: E402
from test_gpu_ops import close, dev, to_dev, T        # noqa: E402

_REF = {}
DROP_P = 0.25


def _ref(name, concat=False, keep_seed=None, g_only=False):
    """The restatement of a case on every side of its data, differentiated once: dict(p (leaves with .grad), g, hs [per side][per
    step], gs [per step] (all sides), cg, ca, cgs, keep (row masks or None)).  The scalar is <g, cg> + 0.1 <h_T, ca[side]>, for the
    dev form also + 0.1 <h_1, ca0[side]> + sum_t <g_t, cgs[t]> (so that the readout layers are reached); ``g_only``: <g, cg> alone."""
    key = (name, concat, keep_seed, g_only)
    if key in _REF:
        return _REF[key]
    c = R.CASES[name]
    d = R.data(c["data"])
    p = {k: v.requires_grad_() for k, v in R.case_params(c, concat).items()}
    kr = None if keep_seed is None else R.keep_rows(c["data"], c["hidden"], c["layers"], keep_seed, DROP_P)
    outs = []
    for side, (atoms, adj) in enumerate(d["sides"]):
        kd = None if kr is None else R.keep_dense(c["data"], kr, side)
        outs.append(R.case_forward(c, p, atoms, adj, concat, step_keep=kd))
    g = torch.cat([o[0] for o in outs])
    gs = [torch.cat([o[2][t] for o in outs]) for t in range(len(outs[0][2]))]
    gen = torch.Generator().manual_seed(5)
    rn = lambda x: torch.randn(x.shape, dtype=torch.float64, generator=gen)
    cg = rn(g)
    ca = [rn(o[1][-1]) for o in outs]
    ca0 = [rn(o[1][0]) for o in outs]
    cgs = [rn(x) for x in gs]
    s = (g * cg).sum()
    if not g_only:
        s = s + 0.1 * sum((o[1][-1] * w).sum() for o, w in zip(outs, ca))
        if c["kind"] == "dev":
            s = s + 0.1 * sum((o[1][0] * w).sum() for o, w in zip(outs, ca0)) + sum((x * w).sum() for x, w in zip(gs, cgs))
    s.backward()
    _REF[key] = dict(p=p, g=g.detach(), hs=[[h.detach() for h in o[1]] for o in outs], gs=[x.detach() for x in gs], cg=cg, ca=ca,
                     ca0=ca0, cgs=cgs, keep=kr)
    return _REF[key]


def _enc(name, concat=False, fused=True, dropout_rate=0.0):
    from bmp.ggnn_dev import DevGGNN, SelfLoopGGNN
    from bmp.snapshot import load_param_dict
    c = R.CASES[name]
    cls = DevGGNN if c["kind"] == "dev" else SelfLoopGGNN
    enc = cls(out_dim=c["out"], hidden_dim=c["hidden"], n_layers=c["layers"], concat_hidden=concat, weight_tying=c["tying"],
              dropout_rate=dropout_rate).to(dev())
    load_param_dict(enc, R.case_params(c, concat))
    if c["kind"] == "loop":
        enc._fused = fused
    return enc


def _run(enc, r, *args):
    """Self-loop form: forward on ``args`` + the backward of the reference's scalar; (g, [dense last atom states per side], grads)."""
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
        close(a, r["hs"][s][-1], f"{tag}atoms {s + 1}")
    assert sorted(gd) == sorted(r["p"])
    for k, gr in gd.items():         # (the first call reads neither W_r nor the U links: a 1-layer case leaves them without gradient)
        want = r["p"][k].grad
        close(gr, want if want is not None else torch.zeros_like(r["p"][k]), f"{tag}grad {k}")


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.LOOP_PATHS)
    out = fn()
    return out, {k: Fn.LOOP_PATHS[k] - before[k] for k in before}


def _pb(name):
    return to_dev(R.data(R.CASES[name]["data"])["pb"])


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("name,path", [("loop16", "composed"), ("loop24", "composed"), ("loop32", "composed"), ("loop64", "fused"),
                                       ("loop128", "fused")])
def test_self_loop_matches_dense_restatement(name, path, concat):
    c = R.CASES[name]
    r = _ref(name, concat)
    enc = _enc(name, concat).eval()
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took == {path: c["layers"], ("composed" if path == "fused" else "fused"): 0}, took
    assert res[0].shape == (26, (c["layers"] if concat else 1) * c["out"])
    _check(res, r)
    assert all(res[2][f"message_self_loop_layers/{k}/W"].abs().max() > 0 for k in range(1 if c["tying"] else c["layers"]))


@pytest.mark.parametrize("name,layers", [("loop64_1", 1), ("loop128_3", 3)])
def test_first_call_alone_and_later_calls(name, layers):
    """One layer: the first-call kernels alone (no r gate, no U term: W_r and the U links get exact zeros).  Three layers: the
    later-call kernels twice, dUcT not zero."""
    assert R.CASES[name]["layers"] == layers
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, _pb(name)))
    assert took == {"fused": layers, "composed": 0}, took
    _check(res, r)
    unread = [k for k in res[2] if k.startswith(("update_layer/U", "update_layer/W_r/"))]
    assert len(unread) == 8
    if layers == 1:
        assert all(res[2][k].abs().max() == 0 for k in unread)
    else:
        assert all(res[2][k].abs().max() > 0 for k in unread)


@pytest.mark.parametrize("name", ["loop64", "loop128", "loop128_3"])
def test_fused_and_composed_paths_agree(name):
    """The fused tile kernels against the existing operators (message operator with its self connection + GRU operator), forced
    through the encoder's private switch, on the same inputs: both float32, different summation orders.  The two runs must really
    take the two paths."""
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


@pytest.mark.parametrize("name", ["loop_over16", "loop_over64"])
def test_molecule_spanning_tiles_takes_the_composed_path(name):
    """One molecule of 150 atoms: its bonds cross the tile boundary, so the tile-local kernels must not run, at a width
    they support (64) as at one they do not (16)."""
    pb = _pb(name)
    assert pb.oversized and pb.max_rows_per_mol == 151
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, pb))
    assert took == {"fused": 0, "composed": 2}, took
    _check(res, r)


@pytest.mark.parametrize("name", ["loop_small16", "loop_small64"])
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


def test_training_dropout_with_given_masks():
    """Training mode at a width the fused kernels support: the step output is dropped, the stateful GRU keeps its un-dropped state --
    the composed operators at every step.  Evaluation mode does not read the masks and takes the fused kernels."""
    name = "loop_drop64"
    steps = R.CASES[name]["layers"]
    r = _ref(name, keep_seed=11)
    pb = _pb(name)
    enc = _enc(name, dropout_rate=DROP_P)
    enc._dropout_masks = [k.to(dev()) for k in r["keep"]]
    assert enc.training
    res, took = _took(lambda: _run(enc, r, pb))
    assert took == {"fused": 0, "composed": steps}, took
    _check(res, r)
    plain = _ref(name)
    ev = _enc(name, dropout_rate=DROP_P).eval()
    ev._dropout_masks = [torch.zeros(pb.n_rows, R.CASES[name]["hidden"], device=dev())] * steps      # must not be read
    out, took = _took(lambda: _run(ev, plain, pb))
    assert took == {"fused": steps, "composed": 0}, took
    _check(out, plain, "eval ")
    assert not torch.equal(out[1][0], res[1][0])
    drawn = _enc(name, dropout_rate=DROP_P)                             # training without given masks: one is drawn per step
    with torch.no_grad():
        drawn(pb)
    assert not torch.equal(drawn.get_atom_array().dense(0), out[1][0])


def _run_dev(enc, r, pb, g_only=False):
    from bmp.snapshot import grad_dict
    d = dev()
    f = lambda x: x.float().to(d)
    g = enc(pb)
    first, last, gl = enc.get_atom_array(0), enc.get_atom_array(-1), enc.get_g_list()
    assert last is enc.get_atom_array() and len(gl) == enc.n_layers
    d0, d1 = [first.dense(s) for s in (0, 1)], [last.dense(s) for s in (0, 1)]
    s = (g * f(r["cg"])).sum()
    if not g_only:
        s = s + 0.1 * sum((a * f(w)).sum() for a, w in zip(d1, r["ca"])) + 0.1 * sum((a * f(w)).sum() for a, w in zip(d0, r["ca0"])) \
            + sum((x * f(w)).sum() for x, w in zip(gl, r["cgs"]))
    s.backward()
    return g.detach(), [a.detach() for a in d0], [a.detach() for a in d1], [x.detach() for x in gl], grad_dict(enc)


def _check_dev(res, r):
    g, d0, d1, gl, gd = res
    close(g, r["g"], "g")
    for s in (0, 1):
        close(d0[s], r["hs"][s][0], f"atoms(0) {s + 1}")
        close(d1[s], r["hs"][s][-1], f"atoms(-1) {s + 1}")
    for t, x in enumerate(gl):
        close(x, r["gs"][t], f"g_list {t}")
    assert sorted(gd) == sorted(r["p"])
    for k, gr in gd.items():
        want = r["p"][k].grad
        close(gr, want if want is not None else torch.zeros_like(r["p"][k]), f"grad {k}")


@pytest.mark.parametrize("name", ["dev16", "dev64", "dev128"])
def test_dev_matches_dense_restatement(name):
    """models/ggnn_dev.py: the returned sum over ALL positions, (26, hidden) wide; get_atom_array(0) / (-1); every entry of
    get_g_list(); gradients of a scalar built from all of them, and of one built from g alone, which never reaches the readout."""
    c = R.CASES[name]
    r = _ref(name)
    res = _run_dev(_enc(name).eval(), r, _pb(name))
    assert res[0].shape == (26, c["hidden"]) and all(x.shape == (26, c["out"]) for x in res[3])
    _check_dev(res, r)
    assert all(res[4][k].abs().max() > 0 for k in res[4] if k.startswith(("i_layers/", "j_layers/")))
    ro = _ref(name, g_only=True)
    only = _run_dev(_enc(name).eval(), ro, _pb(name), g_only=True)
    _check_dev(only, ro)
    assert all(only[4][k].abs().max() == 0 for k in only[4] if k.startswith(("i_layers/", "j_layers/")))


@pytest.mark.parametrize("name", ["dev16", "dev64"])
def test_dev_concat_hidden_returns_the_readouts(name):
    c = R.CASES[name]
    r = _ref(name, concat=True)
    res = _run_dev(_enc(name, concat=True).eval(), r, _pb(name))
    assert res[0].shape == (26, c["layers"] * c["out"]) and torch.equal(res[0], torch.cat(res[3], dim=1))
    _check_dev(res, r)


def test_dev_lists_are_reset_by_every_call():
    enc = _enc("dev16").eval()
    pb = _pb("dev16")
    with torch.no_grad():
        enc(pb)
        a = enc.get_atom_array(0).rows.clone()
        enc(pb)
    assert len(enc.atoms_list) == len(enc.g_vec_list) == 3 and torch.equal(enc.get_atom_array(0).rows, a)


def test_pair_model_one_training_step():
    """Self-loop GGNN + Nie co-attention + MLP as build_pair_predictor builds it (tied, training mode, no dropout): loss, logits and
    every gradient of one eager FlatAdam step against the restatement's."""
    from bmp.dp import FlatAdam
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict
    c = R.CASES["loop_pair16"]
    d = R.data(c["data"])
    hidden, out = c["hidden"], c["out"]
    lab = np.random.RandomState(4).randint(0, 2, (13, 1)).astype(np.int32)
    dr = O._Draw(21, torch.float64, 0.1)
    O.init_nie(dr, "attn/", hidden, out, 8)
    O.init_mlp(dr, "mlp/", 2 * out, 1, (32, 16))
    p = dict(dr.p)
    p.update(R.case_params(c, prefix="graph_conv/"))
    q = {k: v.clone().requires_grad_() for k, v in p.items()}
    at = [R.case_forward(c, q, *d["sides"][s], prefix="graph_conv/")[1][-1] for s in (0, 1)]
    g1, g2 = O.nie_coattention(q, at[0], at[1], "tanh", prefix="attn/")
    y_o = O.mlp_forward(q, torch.cat((g1, g2), dim=-1), 2)
    loss_o = O.sigmoid_cross_entropy(y_o, T(lab))
    names = sorted(q)
    gr = torch.autograd.grad(loss_o, [q[n] for n in names], allow_unused=True)
    g_o = {n: (g if g is not None else torch.zeros_like(q[n])) for n, g in zip(names, gr)}      # (the readout feeds nobody here)
    model = build_pair_predictor(hidden_dim=hidden, out_dim=out, n_layers=c["layers"], attn="nie", encoder="ggnn-self-loop").to(dev())
    load_param_dict(model, p)
    assert model.training
    opt = FlatAdam(model, alpha=1e-2)
    y = opt.functional_forward(_pb("loop_pair16"))
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
