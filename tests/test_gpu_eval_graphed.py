"""Evaluation on recorded graphs with the scores kept on the device (bmp.dp.GraphedPredict + bmp.trainer.ScoreSink) against the
launch-by-launch evaluation through the host: a replay and the eager call run the same kernels on the same arrays, so logits,
metrics and loss are EQUAL; the parameters are read at every replay; a training run does not notice an evaluation in between."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bmp import synth, packed, trainer      # noqa: E402
from test_gpu_ops import dev               # noqa: E402
from parity_util import close              # noqa: E402
from test_gpu_static_batch import CFGS     # noqa: E402

MODELS = {"ref_ntn": CFGS["ref_ntn"], "d64": CFGS["d64"],
          "hole": dict(hidden_dim=32, out_dim=16, n_layers=2, attn=None, sim_method="hole")}


def _model(name, seed=5):
    from bmp.predictor import build_pair_predictor
    from bmp.dp import FlatAdam
    torch.manual_seed(seed)
    model = build_pair_predictor(**MODELS[name]).to(dev())
    return model, FlatAdam(model, alpha=1e-2)


@pytest.fixture(scope="module")
def world():
    store = synth.make_store(40, seed=3, n_lo=3, n_hi=120, n_mean=24)
    ds = packed.DeviceMolStore(packed.MolStore(store), dev())
    rs = np.random.RandomState(8)
    i1, i2 = rs.randint(0, 40, 70), rs.randint(0, 40, 70)
    lab = (np.arange(70) % 3 == 0).astype(np.int32).reshape(70, 1)
    lab[::9] = -1
    return ds, i1, i2, lab


def _batches(world, lo=0, hi=70):
    ds, i1, i2, lab = world
    return trainer.PairBatches(ds, i1[lo:hi], i2[lo:hi], lab[lo:hi], batch_size=32, layout="static")


@pytest.mark.parametrize("name", list(MODELS))
def test_replayed_evaluation_equals_the_eager_one(world, name):
    from bmp.dp import GraphedPredict
    model, opt = _model(name)
    batches = _batches(world)                                   # two fixed-shape batches and a remainder of 6
    assert [len(t) for _, t in batches] == [32, 32, 6]
    host = trainer.evaluate(model, batches, lossfun=model.loss, opt=opt, graphed=False, on_device=False)
    assert not any(np.isnan(v) for v in host.values())
    gp = GraphedPredict(model, opt)
    for kw in (dict(graphed=gp), dict(graphed=True, on_device=True), dict(graphed=False, on_device=True), dict(graphed=gp)):
        got = trainer.evaluate(model, batches, lossfun=model.loss, opt=opt, **kw)
        assert got == host and list(got) == list(host), (kw, got, host)
    assert len(gp.graphs) == 1 and (gp.sink.rows, gp.sink.batches) == (70, 3)       # recorded once, replayed in both passes
    p_host = trainer.predict_pairs(model, batches, opt=opt, graphed=False)
    p_rep = trainer.predict_pairs(model, batches, opt=opt, graphed=True)
    assert sorted(p_rep) == ["labels", "logits", "prob"] and p_rep["logits"].shape == (70, 1)
    for k in p_host:
        assert torch.equal(torch.from_numpy(p_rep[k]), torch.from_numpy(p_host[k])), k
    assert np.array_equal(p_rep["labels"], world[3])
    # a plain replayed predict without a sink: the logits of the recording, valid until the next replay
    plain = GraphedPredict(model, opt)
    n = 0
    for sb, t in batches:
        if callable(getattr(sb, "emit", None)):
            y = plain(sb)
            assert torch.equal(y.cpu(), torch.from_numpy(p_host["logits"][n:n + len(t)]))
        n += len(t)
    assert len(plain.graphs) == 1


def test_the_graph_switch_speaks_for_fixed_shape_sets_and_the_sink_switch_for_the_rest(world, monkeypatch):
    model, opt = _model("hole")
    ds, i1, i2, lab = world
    static, instance = _batches(world), trainer.PairBatches(ds, i1, i2, lab, batch_size=32)
    host = trainer.evaluate(model, static, lossfun=model.loss, opt=opt, graphed=False, on_device=False)
    host_i = trainer.evaluate(model, instance, lossfun=model.loss, opt=opt, graphed=False, on_device=False)
    seen, inner = [], trainer._scores_on_device
    monkeypatch.setattr(trainer, "_scores_on_device", lambda *a, **k: (seen.append(a[4] is not None), inner(*a, **k))[1])
    for graph, sink, want in ((True, False, [True]), (False, True, [False, False]), (False, False, [])):
        monkeypatch.setattr(trainer, "EVAL_GRAPH_DEFAULT", graph)
        monkeypatch.setattr(trainer, "EVAL_ON_DEVICE_DEFAULT", sink)
        del seen[:]
        assert trainer.evaluate(model, static, lossfun=model.loss, opt=opt) == host
        assert trainer.evaluate(model, instance, lossfun=model.loss, opt=opt) == host_i
        assert seen == want, (graph, sink, seen)


def test_what_the_static_layout_refuses_stays_refused_with_its_reason(world, monkeypatch):
    from bmp.predictor import build_pair_predictor
    from bmp.dp import FlatAdam
    torch.manual_seed(5)
    model = build_pair_predictor(hidden_dim=16, out_dim=16, n_layers=2, attn=None, encoder="ggnn-edge").to(dev())
    opt = FlatAdam(model)
    batches = _batches(world)
    with pytest.raises(NotImplementedError, match="edge_network"):
        batches.check_encoder(model)
    for call in (lambda: trainer.evaluate(model, batches, opt=opt, graphed=True),
                 lambda: trainer.predict_pairs(model, batches, opt=opt, graphed=True)):
        with pytest.raises(NotImplementedError, match="edge_network"):
            call()
    monkeypatch.setattr(trainer, "EVAL_GRAPH_DEFAULT", True)           # by default nothing is recorded for such a model
    assert not trainer._graph_by_default(batches, opt, model)


def test_a_set_without_a_size_grows_its_sink_between_batches(world, monkeypatch):
    """A plain list of batches has no pair count: the sink starts small and is doubled twice on the way (32 -> 64 -> 128 rows,
    1 -> 2 -> 4 batches), contents and cursor carried over on the device."""
    model, opt = _model("hole")
    ds, i1, i2, lab = world
    batches = list(trainer.PairBatches(ds, i1, i2, lab, batch_size=32))
    assert [len(t) for _, t in batches] == [32, 32, 6]
    host = trainer.evaluate(model, batches, lossfun=model.loss, opt=opt, on_device=False)
    made, inner = [], trainer.ScoreSink
    monkeypatch.setattr(trainer, "UNSIZED_START", (8, 1))
    monkeypatch.setattr(trainer, "ScoreSink", lambda *a, **k: (made.append(a[1:3]), inner(*a, **k))[1])
    assert trainer.evaluate(model, batches, lossfun=model.loss, opt=opt, on_device=True) == host
    assert made == [(32, 1), (64, 2), (128, 4)], made


def test_a_replay_reads_the_parameters_of_the_moment(world):
    from bmp.dp import GraphedPredict, GraphedTrainStep
    model, opt = _model("d64")
    batches, train = _batches(world), _batches(world, 0, 64)
    gp = GraphedPredict(model, opt)
    first = trainer.evaluate(model, batches, lossfun=model.loss, opt=opt, graphed=gp)
    stepper = GraphedTrainStep(model, opt)
    for sb, _t in train:
        stepper(sb)
        break
    assert opt.t == 1
    second = trainer.evaluate(model, batches, lossfun=model.loss, opt=opt, graphed=gp)
    eager = trainer.evaluate(model, batches, lossfun=model.loss, opt=opt, graphed=False, on_device=False)
    assert second == eager, (second, eager)
    assert second["loss"] != first["loss"]
    assert len(gp.graphs) == 1


def test_training_does_not_notice_an_evaluation_between_its_steps(world):
    from bmp.dp import GraphedTrainStep
    runs = []
    for with_eval in (False, True):
        model, opt = _model("d64")
        ds, i1, i2, lab = world
        valid = _batches(world, 6, 70)
        stepper = GraphedTrainStep(model, opt)
        model.train()
        sb = packed.StaticPairBatch(ds, 32)
        for k in range(3):
            sl = slice(32 * (k % 2), 32 * (k % 2) + 32)
            sb.load([i1[sl], i2[sl]], lab[sl])
            stepper(sb)
            if with_eval and k == 0:
                trainer.evaluate(model, valid, lossfun=model.loss, opt=opt, graphed=True, on_device=True)
                assert model.training
        runs.append((opt.flat.clone(), opt.m.clone(), opt.v.clone(), opt.t))
    a, b = runs
    assert a[3] == b[3] == 3
    for x, y, what in zip(a[:3], b[:3], ("flat", "m", "v")):
        assert torch.equal(x, y), what


def _same(a, b):
    return a == b or (a != a and b != b)


def test_fit_logs_are_the_same_with_the_switches_on_and_off(world, monkeypatch):
    logs = []
    for on in (True, False):
        monkeypatch.setattr(trainer, "EVAL_GRAPH_DEFAULT", on)
        monkeypatch.setattr(trainer, "EVAL_ON_DEVICE_DEFAULT", on)
        model, opt = _model("d64")
        logs.append(trainer.fit(model, opt, _batches(world), _batches(world, 20, 70), epochs=2, eval_train=True))
    on, off = logs
    assert len(on) == len(off) == 2
    for lo, lf in zip(on, off):
        assert list(lo) == list(lf) and "val_roc/main/roc_auc" in lo and "train_roc/main/roc_auc" in lo
        for k in lo:
            if k != "elapsed_time":
                assert _same(lo[k], lf[k]), (k, lo[k], lf[k])
    assert on[0]["validation/main/loss"] != on[1]["validation/main/loss"]


def test_representations_are_the_molecule_vectors_of_every_pair(world):
    model, opt = _model("ref_ntn")
    batches = _batches(world)
    out = trainer.predict_pairs(model, batches, opt=opt, representations=True, graphed=True)
    assert sorted(out) == ["g1", "g2", "labels", "logits", "prob"]
    g1s, g2s, p1s, p2s = [], [], [], []
    model.eval()
    for inputs, _t in batches:
        if callable(getattr(inputs, "emit", None)):
            inputs.reset_derived(); inputs.emit()
            inputs = inputs.pb
        _y, (g1, g2) = opt.functional_predict(inputs)            # predict_eval on the planned path: the same kernels
        g1s.append(g1.clone()); g2s.append(g2.clone())
        _y, (g1, g2) = model.predict_eval(inputs)               # eval_coattention.py:103-124 as the module runs it
        p1s.append(g1.clone()); p2s.append(g2.clone())
    assert torch.equal(torch.from_numpy(out["g1"]), torch.cat(g1s).cpu()) and torch.equal(torch.from_numpy(out["g2"]), torch.cat(g2s).cpu())
    close(torch.from_numpy(out["g1"]), torch.cat(p1s), "predict_pairs g1 against predict_eval", tol=1e-5)
    close(torch.from_numpy(out["g2"]), torch.cat(p2s), "predict_pairs g2 against predict_eval", tol=1e-5)
    assert out["g1"].shape == (70, 16)
