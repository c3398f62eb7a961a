"""Chainer's optimizer hooks for ``bmp.dp.FlatAdam`` (train_binary.py:538-543, and the same block in eight more trainer
scripts): ``optimizer.add_hook(GradientClipping(max_norm))``, ``WeightDecay(l2_rate)``, ``Lasso(l1_rate)``.

Hooks run before the update rule, in the order they were added, each on the gradient as the hooks before it left it.  ``g``
is the flat gradient the update sees (after ``all_reduce_grads`` and its 1/W):

* ``GradientClipping(threshold)``: ``g *= min(1, threshold / sqrt(sum g^2))`` in fp32; a zero norm gives 1;
* ``WeightDecay(rate)``: ``g += rate * p`` (``p`` before this step's update) -- unlike Adam's own ``weight_decay_rate``,
  which is decoupled from the moments;
* ``Lasso(rate)``: ``g += rate * sign(p)``, ``sign(0) = 0``.

On the GPU the hooks and Adam are two launches (``bmp_grad_sumsq_partials`` when a clip is set, then
``bmp_adam_step_hooked``); on the CPU, ``apply_cpu`` in fp32 torch ops.
"""
from __future__ import annotations

from typing import Iterable, Tuple

import torch

# hook codes of the C ABI's hook_order (include/bmp.h)
CLIP, DECAY, LASSO = 1, 2, 3
SUMSQ_PARTS_MAX = 256           # floats of bmp_grad_sumsq_partials' partials buffer, for any n


class GradientClipping:
    """chainer.optimizer_hooks.GradientClipping: rescale the whole gradient to an L2 norm of at most ``threshold``."""
    name = "GradientClipping"
    code = CLIP

    def __init__(self, threshold: float):
        self.threshold = threshold


class WeightDecay:
    """chainer.optimizer_hooks.WeightDecay: ``g += rate * p`` before the moments."""
    name = "WeightDecay"
    code = DECAY

    def __init__(self, rate: float):
        self.rate = rate


class Lasso:
    """chainer.optimizer_hooks.Lasso: ``g += rate * sign(p)`` before the moments."""
    name = "Lasso"
    code = LASSO

    def __init__(self, rate: float):
        self.rate = rate


HOOK_TYPES = (GradientClipping, WeightDecay, Lasso)


def hook_order(hooks: Iterable) -> int:
    """The hooks' kinds in order as the C ABI's 2-bit codes (first hook in the low bits; 0 for no hooks)."""
    order = 0
    for k, h in enumerate(hooks):
        order |= h.code << (2 * k)
    return order


def hook_values(hooks: Iterable) -> Tuple[float, float, float]:
    """(threshold, l2 rate, l1 rate) of the hooks present, 0 for an absent kind."""
    vals = [0.0, 0.0, 0.0]
    for h in hooks:
        vals[h.code - 1] = float(h.threshold if h.code == CLIP else h.rate)
    return vals[0], vals[1], vals[2]


def apply_cpu(g: torch.Tensor, p: torch.Tensor, hooks: Iterable) -> torch.Tensor:
    """The hooked gradient in fp32 torch ops (a new tensor: ``g`` is left alone, as the GPU kernels leave it)."""
    for h in hooks:
        if h.code == CLIP:
            norm = torch.linalg.vector_norm(g)
            g = g * torch.clamp(torch.tensor(h.threshold, dtype=g.dtype) / norm, max=1.0)
        elif h.code == DECAY:
            g = g + h.rate * p
        else:
            g = g + h.rate * torch.sign(p)
    return g
