"""GPU parity tests of the fuse-gate and simple-gate GGNN encoders at hidden width 32 (bmp/ggnn_gate.py on the wave-local step
kernels of csrc/bmp_gate_small.hip) against the float64 dense restatement (tests/ggate_ref.py through tests/ggate32_ref.py): g,
get_atom_array().dense(side) and every parameter gradient at max-norm 1e-4 through parity_util.close.  Every case takes its
(kind, seed, shape, data) from ggate32_ref.CASES; the references are computed once per (case, options) and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ggate32_ref as R                               # noqa: E402
from bmp import packed                                # noqa: E402
from test_gpu_ops import close, dev, to_dev, T        # noqa: E402

_REF = {}


def _ref(name, concat=False, keep_seed=None):
    key = (name, concat, keep_seed)
    if key not in _REF:
        _REF[key] = R.reference(name, concat, keep_seed)
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


def _path(name):
    """The form Fn.gate_step picks for the case's kind at d = 32 on whole tiles: the table the measurement filled."""
    from bmp import functional as Fn
    return "fused" if Fn.GATE_SMALL_DEFAULT[R.CASES[name]["kind"]] else "composed"


@pytest.fixture
def small_on(monkeypatch):
    """Both kinds on the d = 32 kernels, whatever the dispatch table says: the kernels are tested either way."""
    from bmp import functional as Fn
    monkeypatch.setattr(Fn, "GATE_SMALL_DEFAULT", {"fuse": True, "gate": True})


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("name", ["fuse32", "gate32", "gate32u", "fuse_keep32", "fuse_blocks32", "gate_blocks32", "fuse_dense32",
                                  "gate_dense32"])
def test_matches_dense_restatement(name, concat, small_on):
    c = R.CASES[name]
    if c["data"] == "blocks":
        assert R.blocks_property(R.data("blocks")["pb"])
    if c["data"] == "dense":         # more CSR entries than fit the staging: both directions gather from global memory
        assert R.dense_property(R.data("dense")["pb"])
    r = _ref(name, concat)
    enc = _enc(name, concat).eval()
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took == {"fused": c["layers"], "composed": 0}, took
    assert res[0].shape == (R.data(c["data"])["pb"].n_mols, (c["layers"] if concat else 1) * c["out"])
    _check(res, r)
    if c["kind"] == "fuse":          # the links nobody calls get no gradient
        assert all(v.abs().max() == 0 for k, v in res[2].items() if k.startswith("update_layer/") or k.startswith("embed_linear/"))


@pytest.mark.parametrize("name", ["fuse32", "gate32"])
def test_dispatch_follows_the_measured_table(name):
    """Without the override: Fn.gate_step sends a kind to the d = 32 kernels iff GATE_SMALL_DEFAULT says so."""
    r = _ref(name)
    steps = R.CASES[name]["layers"]
    res, took = _took(lambda: _run(_enc(name).eval(), r, _pb(name)))
    other = "composed" if _path(name) == "fused" else "fused"
    assert took == {_path(name): steps, other: 0}, took
    _check(res, r)


@pytest.mark.parametrize("name", ["fuse32", "gate32", "fuse_blocks32", "gate_blocks32", "fuse_dense32"])
def test_fused_and_composed_paths_agree(name, small_on):
    """The d = 32 kernels against the existing operators (message operator + row linear + torch elementwise), forced through
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
    for s in range(len(res[0][1])):
        close(res[0][1][s], res[1][1][s], f"fused vs composed atoms {s + 1}")
    for k in res[0][2]:
        close(res[0][2][k], res[1][2][k], f"fused vs composed grad {k}")
    assert not torch.equal(res[0][1][0], res[1][1][0])


def test_fuse_training_mode_with_given_masks(small_on):
    """Training mode: the fuse gate's dropout on r * h with the masks given (ratio 0.05: 1 / 0.95 or 0); evaluation mode does not
    read them."""
    name = "fuse_keep32"
    r = _ref(name, keep_seed=11)
    pb = _pb(name)
    enc = _enc(name)
    enc._dropout_masks = [k.to(dev()) for k in r["keep"]]
    assert enc.training
    res, took = _took(lambda: _run(enc, r, pb))
    assert took == {"fused": 2, "composed": 0}, took
    _check(res, r)
    plain = _ref(name)
    ev = _enc(name).eval()
    ev._dropout_masks = [torch.zeros(pb.n_rows, 32, device=dev())] * 2       # must not be read
    out = _run(ev, plain, pb)
    _check(out, plain, "eval ")
    assert not torch.equal(out[1][0], res[1][0])


def test_gate_with_untied_update_layers(small_on):
    name = "gate32u"
    r = _ref(name)
    enc = _enc(name)
    assert len(enc.gate_layer) == 3 and not enc.update_tying
    res, took = _took(lambda: _run(enc, r, _pb(name)))
    assert took == {"fused": 3, "composed": 0}, took
    _check(res, r)
    assert all(res[2][f"gate_layer/{k}/W"].abs().max() > 0 for k in range(3))


@pytest.mark.parametrize("name", ["fuse_over32", "gate_over32"])
def test_molecule_spanning_tiles_takes_the_composed_path(name, small_on):
    """One molecule of 150 atoms: its bonds cross the tile boundary, so the tile-local kernels must not run."""
    pb = _pb(name)
    assert pb.oversized and pb.max_rows_per_mol == 151
    r = _ref(name)
    res, took = _took(lambda: _run(_enc(name).eval(), r, pb))
    assert took == {"fused": 0, "composed": 2}, took
    _check(res, r)


def test_dense_call_form_equals_packed_form(small_on):
    name = "fuse_small32"
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


@pytest.mark.parametrize("name", ["fuse32", "gate_blocks32"])
def test_forward_only_form_is_bit_identical(name, small_on):
    """Under torch.no_grad() the step passes null m and act (the instance that saves nothing): the same values, bit for bit, as
    the forward of the training form."""
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


@pytest.mark.parametrize("name", ["fuse_keep32", "gate_blocks32"])
def test_two_runs_give_bit_identical_gradients(name, small_on):
    keep_seed = 11 if name == "fuse_keep32" else None
    r = _ref(name, keep_seed=keep_seed)
    res = []
    for _ in range(2):
        enc = _enc(name)
        if keep_seed is not None:
            enc._dropout_masks = [k.to(dev()) for k in r["keep"]]
        else:
            enc.eval()
        res.append(_run(enc, r, _pb(name)))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


def _step_operands(kind, d, n_tiles=1):
    """Operands of one direct call of the small entries on an edgeless tile (every pointer valid and 16-byte aligned)."""
    from bmp._lib import ptr
    nu = (3 if kind == 0 else 1) * d
    N = 128 * n_tiles
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev())
    o = dict(h=f(N, d), WTp=f(4 * d, d), bE=f(4, d), AUp=f(2 * d, nu), bU=f(nu), m=f(N, d), act=f(N, nu), hout=f(N, d) + 7.0,
             dhout=f(N, d), Wnp=f(d, 4 * d), Unp=f(nu, 2 * d), dh=f(N, d) + 7.0, gda=f(N, 4 * d + nu) + 7.0,
             cp=torch.zeros(N + 1, dtype=torch.int32, device=dev()), cc=torch.zeros(4, dtype=torch.int32, device=dev()), cv=f(4))
    return o, {k: ptr(v) for k, v in o.items()}


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("fault", ["width", "misaligned"])
def test_small_entries_refuse_bad_arguments_without_launching(kind, fault):
    """d = 64, or a pointer 4 bytes off a 16-byte boundary: the entries answer with the library's argument-check error, which
    ``check`` raises (its ValueError, "argument check failed": bmp/_lib.py), and launch nothing -- the outputs keep their fill."""
    from bmp import _lib
    from bmp._lib import check, stream
    L = _lib.lib()
    d = 64 if fault == "width" else 32
    o, p = _step_operands(kind, d)
    off = 4 if fault == "misaligned" else 0
    with pytest.raises(ValueError, match="bmp_ggnn_gate_step_small_fwd: argument check failed"):
        check(L.bmp_ggnn_gate_step_small_fwd(kind, p["h"] + off, 1, d, p["cp"], p["cc"], p["cv"], p["WTp"], p["bE"], p["AUp"], p["bU"],
                                             None, p["m"], p["act"], p["hout"], stream()), "bmp_ggnn_gate_step_small_fwd")
    with pytest.raises(ValueError, match="bmp_ggnn_gate_step_small_bwd: argument check failed"):
        check(L.bmp_ggnn_gate_step_small_bwd(kind, p["dhout"], p["h"], p["m"], p["act"], None, 1, d, p["cp"], p["cc"], p["cv"],
                                             p["Wnp"], p["Unp"], p["dh"], p["gda"] + off, stream()), "bmp_ggnn_gate_step_small_bwd")
    if fault == "width":             # m given without act: refused too
        o32, q = _step_operands(kind, 32)
        with pytest.raises(ValueError, match="argument check failed"):
            check(L.bmp_ggnn_gate_step_small_fwd(kind, q["h"], 1, 32, q["cp"], q["cc"], q["cv"], q["WTp"], q["bE"], q["AUp"], q["bU"],
                                                 None, q["m"], None, q["hout"], stream()), "bmp_ggnn_gate_step_small_fwd")
        assert (o32["hout"] == 7.0).all()
    torch.cuda.synchronize()
    assert (o["hout"] == 7.0).all() and (o["dh"] == 7.0).all() and (o["gda"] == 7.0).all()


def test_gate_step_fn_refuses_other_widths():
    from bmp import functional as Fn
    pb = _pb("fuse32")
    d = 16
    z = lambda *s: torch.zeros(*s, device=dev())
    with pytest.raises(ValueError, match=r"\{32, 64, 128\}"):
        Fn.GateStepFn.apply(z(pb.n_rows, d), z(4 * d, d), z(4, d), z(2 * d, 3 * d), z(3 * d), None, pb, 0)


def test_pair_model_one_training_step(small_on):
    """The recorded model shape cut down (RECORD.txt:404-405): fuse-gate encoder at d = 32, 2 untied layers, no co-attention, HolE
    link predictor, training mode with the masks given.  Loss, logits and every gradient of one eager FlatAdam step against the
    restatement (ggate_ref's encoder, link_ref's circular correlation)."""
    from bmp.dp import FlatAdam
    from bmp.ggnn_gate import FuseGGNN
    from bmp.predictor import GraphConvPredictorForPair, build_link_predictor
    from bmp.snapshot import load_param_dict
    c = R.CASES[R.PAIR_CASE]
    ref = R.pair_reference()
    enc = FuseGGNN(out_dim=c["out"], hidden_dim=c["hidden"], n_layers=c["layers"], weight_tying=c["tying"])
    model = GraphConvPredictorForPair(enc, None, build_link_predictor("hole", c["out"], 1, R.PAIR_HIDDEN_DIMS)).to(dev())
    load_param_dict(model, R.pair_params())
    model.graph_conv._dropout_masks = [k.to(dev()) for k in ref["keep"]]
    assert model.training
    opt = FlatAdam(model, alpha=1e-2)
    lab = T(R.pair_labels()).to(dev())
    (y, took) = _took(lambda: opt.functional_forward(_pb(R.PAIR_CASE)))
    assert took == {"fused": c["layers"], "composed": 0}, took
    loss = model.loss(y, lab)
    loss.backward()
    opt.collect_grads()
    close(y, ref["y"], "logits"); close(loss, ref["loss"], "loss")
    off, seen = 0, set()
    for name, shp in zip(opt.names, opt.shapes):
        n = int(np.prod(shp))
        key = name.replace(".", "/")
        close(opt.grad[off:off + n].view(shp), ref["grads"][key], f"grad {name}")
        seen.add(key)
        off += n
    assert seen == set(ref["grads"])
    before = opt.flat.clone()
    opt.step()
    assert torch.isfinite(opt.flat).all() and not torch.equal(opt.flat, before)
