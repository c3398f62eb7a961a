"""GPU parity tests of the GGNN with message_function='edge_network' (bmp/ggnn.py, Fn.edge_step, csrc/bmp_edge.hip) against the
float64 dense restatement (tests/edge_ref.py): molecule vectors, atom arrays and every parameter gradient at max-norm 1e-4 through
parity_util.close (the float32 restatement lies within 4.5e-6 of the float64 one on these shapes, forward and gradients: the
figures stand beside edge_ref.CASES).  Every case takes its (seed, shape, data) from edge_ref.CASES; the references are computed
once per (case, options) and shared; the path counters say which form every step took."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edge_ref as R                                  # noqa: E402
from oracle import ref_cpu as O                       # noqa: E402
from bmp import packed                                # noqa: E402
from test_gpu_ops import close, dev, to_dev, T        # noqa: E402

_REF = {}
DROP_P = 0.25


def _ref(name, concat=False, keep_seed=None, aggregator=None, sides=None):
    """The restatement of a case on every side of its data (or on the given ``sides``), differentiated once: dict(p (leaves with
    .grad), g, hs [per side] (last atom states), cg, ca, keep (row masks or None)).  The scalar is <g, cg> + 0.1 <h_T, ca[side]>."""
    key = (name, concat, keep_seed, aggregator, None if sides is None else id(sides))
    if key in _REF:
        return _REF[key]
    c = R.CASES[name]
    p = {k: v.requires_grad_() for k, v in R.case_params(c, concat, aggregator=aggregator).items()}
    kr = None if keep_seed is None else R.keep_rows(c["data"], c["hidden"], c["layers"], keep_seed, DROP_P)
    outs = []
    for side, (atoms, adj) in enumerate(R.data(c["data"])["sides"] if sides is None else sides):
        kd = None if kr is None else R.keep_dense(c["data"], kr, side)
        outs.append(R.case_forward(c, p, atoms, adj, concat, step_keep=kd, aggregator=aggregator))
    g = torch.cat([o[0] for o in outs])
    gen = torch.Generator().manual_seed(5)
    rn = lambda x: torch.randn(x.shape, dtype=torch.float64, generator=gen)
    cg = rn(g)
    ca = [rn(o[1][-1]) for o in outs]
    s = (g * cg).sum()
    if not aggregator:              # (with an aggregator the encoder hands over no atom array)
        s = s + 0.1 * sum((o[1][-1] * w).sum() for o, w in zip(outs, ca))
    s.backward()
    _REF[key] = dict(p=p, g=g.detach(), hs=[o[1][-1].detach() for o in outs], cg=cg, ca=ca, keep=kr, sides=sides)
    return _REF[key]


def _enc(name, concat=False, fused=True, dropout_rate=0.0, aggregator=None):
    from bmp.ggnn import GGNN
    from bmp.snapshot import load_param_dict
    c = R.CASES[name]
    enc = GGNN(out_dim=c["out"], hidden_dim=c["hidden"], n_layers=c["layers"], concat_hidden=concat, weight_tying=c["tying"],
               dropout_rate=dropout_rate, message_function='edge_network', layer_aggregator=aggregator).to(dev())
    load_param_dict(enc, R.case_params(c, concat, aggregator=aggregator))
    enc.fused = fused
    return enc


def _run(enc, r, *args):
    """Forward on ``args`` + the backward of the reference's scalar; (g, [dense last atom states per side], grads)."""
    from bmp.snapshot import grad_dict
    g = enc(*args)
    d = dev()
    s = (g * r["cg"].float().to(d)).sum()
    dn = []
    if not enc.layer_aggregator:
        at = enc.get_atom_array()
        dn = [at.dense(k) for k in range(len(r["ca"]))]
        s = s + 0.1 * sum((a * w.float().to(d)).sum() for a, w in zip(dn, r["ca"]))
    s.backward()
    return g.detach(), [a.detach() for a in dn], grad_dict(enc)


def _check(res, r, tag=""):
    g, dn, gd = res
    close(g, r["g"], tag + "g")
    for s, a in enumerate(dn):
        close(a, r["hs"][s], f"{tag}atoms {s + 1}")
    assert sorted(gd) == sorted(r["p"])
    for k, gr in gd.items():         # (never read: hidden_layers/0 always; W_r and the U links in a 1-layer case)
        want = r["p"][k].grad
        close(gr, want if want is not None else torch.zeros_like(r["p"][k]), f"{tag}grad {k}")
    assert all(gd[k].abs().max() == 0 for k in gd if "hidden_layers" in k)
    assert all(gd[k].abs().max() > 0 for k in gd if k.endswith("output_layer/b"))
    # (W_e meets bonds only: the one-atom molecules of "many" have none, and the restatement says so too)
    assert all((gd[k].abs().max() > 0) == (r["p"][k].grad.abs().max() > 0) for k in gd if k.endswith("output_layer/W"))


def _took(fn):
    from bmp import functional as Fn
    before = dict(Fn.EDGE_PATHS)
    out = fn()
    return out, {k: Fn.EDGE_PATHS[k] - before[k] for k in before}


def _pb(name):
    return to_dev(R.data(R.CASES[name]["data"])["pb"])


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("name,path", [("edge16", "composed"), ("edge24", "composed"), ("edge32", "composed"), ("edge64", "fused"),
                                       ("edge128", "fused")])
def test_matches_dense_restatement(name, path, concat):
    c = R.CASES[name]
    r = _ref(name, concat)
    enc = _enc(name, concat).eval()
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took == {path: c["layers"], ("composed" if path == "fused" else "fused"): 0}, took
    assert res[0].shape == (26, (c["layers"] if concat else 1) * c["out"])
    _check(res, r)


@pytest.mark.parametrize("name,layers", [("edge64_1", 1), ("edge128_1", 1), ("edge64_3", 3), ("edge128_3", 3)])
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


@pytest.mark.parametrize("name", ["edge_many64", "edge_many128", "edge_full64", "edge_full128"])
def test_segment_sum_at_its_edges(name):
    """The in-tile segment sum with 64 segments of two rows in one tile ("many") and with ONE segment that is the whole tile --
    127 atoms and the pad row -- beside a tile of small molecules whose pad rows count 115 times and more ("full")."""
    pb = _pb(name)
    assert not pb.oversized and int(pb.mol_nrows.max()) == (2 if "many" in name else 128)
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, pb))
    assert took == {"fused": R.CASES[name]["layers"], "composed": 0}, took
    _check(res, r)


@pytest.mark.parametrize("name", ["edge_over16", "edge_over64"])
def test_molecule_spanning_tiles_takes_the_composed_path(name):
    """One molecule of 150 atoms: its bonds and its segment cross the tile boundary, so the tile-local kernels must not run, at a
    width they support (64) as at one they do not (16)."""
    pb = _pb(name)
    assert pb.oversized and pb.max_rows_per_mol == 151
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, pb))
    assert took == {"fused": 0, "composed": 2}, took
    _check(res, r)


def _padded(atoms, adj, k):
    mb, A = atoms.shape
    a = np.zeros((mb, A + k), np.int32); a[:, :A] = atoms
    j = np.zeros((mb, 4, A + k, A + k), np.float32); j[:, :, :A, :A] = adj
    return a, j


_SMALL_PADDED = [_padded(*R.data("small")["sides"][0], 3)]


@pytest.mark.parametrize("name", ["edge_small16", "edge_small64"])
def test_dense_call_form_at_two_paddings(name):
    """The reference's call form (atoms (mb, A), adj (mb, 4, A, A)): equal to the packed form bit for bit, and, padded to A + 3,
    equal to the restatement AT THAT PADDING -- the real atoms' states move with A for this message function."""
    atoms, adj = R.data("small")["sides"][0]
    r = _ref(name)
    pb = packed.pack_from_dense([atoms], [adj], device=dev())
    a = _run(_enc(name).eval(), r, pb)
    b = _run(_enc(name).eval(), r, atoms, adj)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    _check(a, r)
    a3, j3 = _SMALL_PADDED[0]
    r3 = _ref(name, sides=_SMALL_PADDED)
    res3 = _run(_enc(name).eval(), r3, a3, j3)
    _check(res3, r3, "A + 3: ")
    A = atoms.shape[1]
    real = torch.as_tensor(atoms != 0)
    assert (res3[1][0][:, :A].cpu()[real] - a[1][0].cpu()[real]).abs().max() > 1e-3


@pytest.mark.parametrize("name", ["edge64", "edge128", "edge128_3"])
def test_fused_and_composed_paths_agree(name):
    """The fused tile kernels against the existing operators (message operator, segment pool, row broadcast, GRU operator), forced
    through the encoder's ``fused`` switch, on the same inputs: both float32, different summation orders.  The two runs must really
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


def test_training_dropout_with_given_masks():
    """Training mode at a width the fused kernels support: the step output is dropped, the stateful GRU keeps its un-dropped state --
    the composed operators at every step.  Evaluation mode does not read the masks and takes the fused kernels."""
    name = "edge_drop64"
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


def test_attn_layer_aggregator_on_top():
    name = "edge_attn64"
    r = _ref(name, aggregator="attn")
    enc = _enc(name, aggregator="attn").eval()
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took == {"fused": R.CASES[name]["layers"], "composed": 0}, took
    _check(res, r)
    assert res[2]["attn_dense_layer/W"].abs().max() > 0
    with pytest.raises(RuntimeError):
        enc.get_atom_array()


@pytest.mark.parametrize("name", ["edge64", "edge128"])
def test_forward_under_no_grad(name):
    """Forward-only evaluation: the kernels are handed no m / r|z / c arrays to fill (nothing is saved), and give the same states."""
    r = _ref(name)
    pb = _pb(name)
    enc = _enc(name).eval()
    with torch.no_grad():
        (g, took) = _took(lambda: enc(pb))
    assert took == {"fused": R.CASES[name]["layers"], "composed": 0} and not g.requires_grad
    at = enc.get_atom_array()
    assert at.rows.grad_fn is None
    close(g, r["g"], "no_grad g")
    ref = _run(_enc(name).eval(), r, pb)
    assert torch.equal(g, ref[0]) and torch.equal(at.dense(0), ref[1][0])


def test_zero_bias_equals_the_plain_ggnn():
    """B = 0 and W_e copied from a matrix_multiply GGNN whose message bias is zero: the edge-network encoder and the existing GGNN
    encoder agree on the same batch, fused kernels on both sides (d = 64) and composed operators on both (d = 16)."""
    from bmp.ggnn import GGNN
    from bmp.snapshot import load_param_dict
    for name in ("edge64", "edge16"):
        c = R.CASES[name]
        d, T_ = c["hidden"], c["layers"]
        p = R.case_params(c)
        q = {k: v for k, v in p.items() if "message_layers" not in k}
        gen = torch.Generator().manual_seed(9)
        for i in range(1 if c["tying"] else T_):
            Wm = torch.randn(4 * d, d, dtype=torch.float64, generator=gen) * (0.5 / d ** 0.5)          # GraphLinear(d, 4d): row 4 c + e
            q[f"message_layers/{i}/W"], q[f"message_layers/{i}/b"] = Wm, torch.zeros(4 * d, dtype=torch.float64)
            p[f"message_layers/{i}/output_layer/W"] = Wm.reshape(d, 4, d).permute(0, 2, 1).reshape(d * d, 4)
            p[f"message_layers/{i}/output_layer/b"] = torch.zeros(d * d, dtype=torch.float64)
        kw = dict(out_dim=c["out"], hidden_dim=d, n_layers=T_, weight_tying=c["tying"])
        edge = GGNN(message_function='edge_network', **kw).to(dev()).eval()
        plain = GGNN(**kw).to(dev()).eval()
        load_param_dict(edge, p); load_param_dict(plain, q)
        pb = _pb(name)
        with torch.no_grad():
            (ge, took) = _took(lambda: edge(pb))
            gp = plain(pb)
        assert took["fused" if d == 64 else "composed"] == T_
        close(ge, gp, f"{name}: g against the plain GGNN")
        close(edge.get_atom_array().rows, plain.get_atom_array().rows, f"{name}: atoms against the plain GGNN")


def test_pair_model_one_training_step():
    """Edge-network GGNN + Nie co-attention + MLP as build_pair_predictor builds it (tied, training mode, no dropout): loss, logits
    and every gradient of one eager FlatAdam step against the restatement's; with a WeightDecay hook the step moves output_layer and
    leaves the never-read hidden_layers.0 bit-identical (Chainer skips parameters without a gradient, hooks included)."""
    from bmp.dp import FlatAdam, WeightDecay
    from bmp.predictor import build_pair_predictor
    from bmp.snapshot import load_param_dict, param_dict
    c = R.CASES["edge_pair16"]
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
    model = build_pair_predictor(hidden_dim=hidden, out_dim=out, n_layers=c["layers"], attn="nie", encoder="ggnn-edge").to(dev())
    load_param_dict(model, p)
    assert model.training
    opt = FlatAdam(model, alpha=1e-2)
    opt.add_hook(WeightDecay(1e-2))
    dead = [n for n in param_dict(model) if "hidden_layers" in n]
    assert len(dead) == 2 and not any(n.replace("/", ".") in opt.names for n in dead)
    assert sorted(n.replace(".", "/") for n in opt.names) == sorted(set(p) - set(dead))
    y = opt.functional_forward(_pb("edge_pair16"))
    loss = model.loss(y, T(lab).to(dev()))
    loss.backward()
    opt.collect_grads()
    close(y, y_o, "logits"); close(loss, loss_o, "loss")
    off = 0
    for name, shp in zip(opt.names, opt.shapes):
        n = int(np.prod(shp))
        close(opt.grad[off:off + n].view(shp), g_o[name.replace(".", "/")], f"grad {name}")
        off += n
    before = {k: v.clone() for k, v in param_dict(model).items()}
    opt.step()
    after = param_dict(model)
    assert all(torch.isfinite(v).all() for v in after.values())
    for k in dead:
        assert torch.equal(after[k], before[k]) and torch.equal(after[k], p[k].float().to(dev())), k
    for k in ("graph_conv/message_layers/0/output_layer/W", "graph_conv/message_layers/0/output_layer/b"):
        assert not torch.equal(after[k], before[k]), k
    # a batch in the encoder layout is refused through encode_rows
    from bmp import enclayout
    eb = enclayout.encode_from_store(packed.MolStore(d["store"]), d["idx"], device=dev())
    with pytest.raises(NotImplementedError, match="padded atom count"):
        model(eb)
