"""CPU checks of the rows-entry protocol that ``bmp.ggnn._StepEncoder`` holds for the six step encoders (bmp/ggnn_gate.py,
bmp/ggnn_dev.py, bmp/ggnn_jk.py): ``rows_reason`` / ``encode_rows`` over every mode, the ``_dropout_masks`` validation, the two
layout attributes ``PairBatches.check_encoder`` probes, and the float-atom refusal with each class's reference lines.

The expected reasons are written out per family from the three ``rows_reason`` bodies the classes had before the protocol moved
into the base (gate: concat_hidden, then the fuse gate in training, then training dropout; dev: concat_hidden, then training
dropout; jk: layout_reason, then concat_hidden, then training dropout), and the texts are spelled out here, not read back."""
import numpy as np
import pytest
import torch

from table_build import enc_batch

CONCAT = ("concat_hidden=True reads out after every step on the per-instance rows; it takes the per-instance "
          "batch form")
FUSE = ("the fuse gate's dropout on r * h is active in training, and the encoder layout (dedup above all) "
        "would give all instances of a molecule one mask; train per-instance or on the static batch, or call "
        "eval()")
DROPOUT = ("dropout_rate > 0 is active in training, and the encoder layout (dedup above all) would give all "
           "instances of a molecule one mask; train per-instance or on the static batch, or call eval()")
ATTN = ("with layer_aggr='attn' the aggregation coefficients are a softmax over inner products taken over ALL atoms and padded positions "
        "of a whole batch side, so a molecule's vector depends on the other molecules of its side and on the padded atom count: one pad "
        "row per tile (the encoder layout), one encoding per distinct molecule (dedup), the layout plan and the recorded step are not "
        "valid for it; use the per-instance batch form")

# (concat_hidden, training, dropout_rate) -> the reason
PLAIN = {(False, False, 0.0): None, (False, False, 0.1): None, (False, True, 0.0): None, (False, True, 0.1): DROPOUT,
         (True, False, 0.0): CONCAT, (True, False, 0.1): CONCAT, (True, True, 0.0): CONCAT, (True, True, 0.1): CONCAT}
FUSED = {(False, False, 0.0): None, (False, False, 0.1): None, (False, True, 0.0): FUSE, (False, True, 0.1): FUSE,
         (True, False, 0.0): CONCAT, (True, False, 0.1): CONCAT, (True, True, 0.0): CONCAT, (True, True, 0.1): CONCAT}
ALWAYS_ATTN = {k: ATTN for k in PLAIN}

# name: (module, class, further constructor arguments, the reasons, the reference lines of the float-atom refusal)
CASES = {
    "fuse": ("ggnn_gate", "FuseGGNN", {}, FUSED, "models/ggnn_dev_fuse.py:149-150, models/ggnn_dev_gate.py:136-137"),
    "gate": ("ggnn_gate", "GateGGNN", {}, PLAIN, "models/ggnn_dev_fuse.py:149-150, models/ggnn_dev_gate.py:136-137"),
    "dev": ("ggnn_dev", "DevGGNN", {}, PLAIN, "models/ggnn_dev.py:140-143, models/ggnn_dev_self_loop.py:125-128"),
    "loop": ("ggnn_dev", "SelfLoopGGNN", {}, PLAIN, "models/ggnn_dev.py:140-143, models/ggnn_dev_self_loop.py:125-128"),
    "jknet_max": ("ggnn_jk", "JKNetGGNN", {"layer_aggr": "max"}, PLAIN, "models/ggnn_dev_jknet.py:158-161"),
    "jknet_attn": ("ggnn_jk", "JKNetGGNN", {"layer_aggr": "attn"}, ALWAYS_ATTN, "models/ggnn_dev_jknet.py:158-161"),
    "jk_gru": ("ggnn_jk", "JKGruGGNN", {}, PLAIN, "models/ggnn_dev_jk_gru.py:135-138"),
}
_EB = {}


def _enc(name, **kw):
    import importlib
    mod, cls, extra = CASES[name][:3]
    return getattr(importlib.import_module("bmp." + mod), cls)(out_dim=8, hidden_dim=64, n_layers=2, **extra, **kw)


def _pb():
    if "eb" not in _EB:
        _EB["eb"] = enc_batch()
    return _EB["eb"].pb_enc


def test_the_reason_constants_read_as_before():
    from bmp import ggnn_gate, ggnn_jk
    assert ggnn_gate.CONCAT_LAYOUT_REASON == CONCAT and ggnn_gate.FUSE_TRAIN_LAYOUT_REASON == FUSE
    assert ggnn_gate.DROPOUT_LAYOUT_REASON == DROPOUT and ggnn_jk.JK_ATTN_LAYOUT_REASON == ATTN


@pytest.mark.parametrize("name", list(CASES))
def test_rows_reason_and_encode_rows_in_every_mode(name):
    pb = _pb()
    for (concat, train, rate), reason in CASES[name][3].items():
        enc = _enc(name, concat_hidden=concat, dropout_rate=rate).train(train)
        assert enc.rows_reason() == reason, (concat, train, rate)
        if reason is not None:
            with pytest.raises(NotImplementedError) as e:
                enc.encode_rows(pb)
            assert str(e.value) == "encode_rows: " + reason, (concat, train, rate)


@pytest.mark.parametrize("name", list(CASES))
def test_layout_attributes_read_as_before(name):
    attn = CASES[name][3] is ALWAYS_ATTN
    for concat in (False, True):
        for train in (False, True):
            enc = _enc(name, concat_hidden=concat, dropout_rate=0.1).train(train)
            assert enc.encoder_layout_reason == (CONCAT if concat else None)
            assert getattr(enc, "layout_reason", None) == (ATTN if attn else None)      # (as check_encoder probes it)
            assert enc.plannable() is False


class _CpuEmbed:
    """Stands in for Fn.EmbedFn (whose table must be on the GPU): zero rows of the right shape."""

    @staticmethod
    def apply(W, ids):
        return torch.zeros(ids.numel(), W.shape[1])


@pytest.mark.parametrize("name", list(CASES))
def test_wrong_dropout_masks_raise_one_text(name, monkeypatch):
    """The masks a test injects are validated once, in the base: a wrong count and a wrong shape raise the same ValueError from the
    call of every class that reads them, before any step runs.  The fuse gate reads them in training whatever dropout_rate is (they
    are its masks on r * h); GateGGNN's call never read them and still does not, so the shared validation is asked directly."""
    from bmp import functional as Fn
    monkeypatch.setattr(Fn, "EmbedFn", _CpuEmbed)
    pb = _pb()
    n = pb.n_rows
    text = f"_dropout_masks: expected 2 tensors of shape ({n}, 64)"
    enc = _enc(name, dropout_rate=0.1).train()
    for e in [enc] + ([_enc(name).train()] if name == "fuse" else []):
        run = (lambda: e._masks(torch.zeros(n, 64))) if name == "gate" else (lambda: e(pb))
        for wrong in ([torch.ones(n, 64)] * 3, [torch.ones(n, 64)], [torch.ones(n, 32)] * 2, [torch.ones(n + 1, 64)] * 2):
            e._dropout_masks = wrong
            with pytest.raises(ValueError) as err:
                run()
            assert str(err.value) == text
    good = [torch.ones(n, 64)] * 2
    enc._dropout_masks = good
    assert enc._masks(torch.zeros(n, 64)) == (True, good)
    enc.eval()
    enc._dropout_masks = [torch.ones(n, 32)]                            # not read under eval()
    assert enc._masks(torch.zeros(n, 64)) == (False, None)


@pytest.mark.parametrize("name", list(CASES))
def test_float_atoms_are_refused_with_the_class_reference_lines(name):
    enc = _enc(name)
    x = np.zeros((2, 3, 64), dtype=np.float32)
    adj = np.zeros((2, 4, 3, 3), dtype=np.float32)
    for atoms in (x, torch.from_numpy(x)):
        with pytest.raises(NotImplementedError) as e:
            enc(atoms, adj)
        assert str(e.value) == f"float atom features (embedding bypass, {CASES[name][4]}) are not supported"
