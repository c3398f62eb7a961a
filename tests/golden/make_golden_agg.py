"""Writes tests/golden/ggnn_agg_{concat,max,attn}.npz: float64 vectors of the layer-aggregator restatement (tests/agg_ref.py)
on a small padded batch -- six synthetic molecules of different sizes plus one with an isolated atom --, d = 16, out 8, for
T = 3 and 4 propagation steps, each with tied and untied message layers.  Per case ``c{T}{t|u}``: the parameters (p:), g,
the gradients of sum(g * gw) with respect to every parameter (d:) and to h0 as an input of its own (dh0: the embedding
output fed in as float features).  The parameters are rounded to float32 before the float64 run, so a float32 model holds
exactly the values the vectors were computed from; parameters and gradients are stored as float32 (the rounding of a stored
gradient, 6e-8, is far inside the 1e-4 the comparisons allow), g and dh0 as float64.  Run from the repository root: python tests/golden/make_golden_agg.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE),
                os.path.join(os.path.dirname(os.path.dirname(HERE)), "gcn-bmp_amd")]
import agg_ref as AR            # noqa: E402
from bmp import synth           # noqa: E402

D, OUT, N_ATOM_TYPES = 16, 8, 18
FILES = {"concat": "ggnn_agg_concat.npz", "max-pool": "ggnn_agg_max.npz", "attn": "ggnn_agg_attn.npz"}
CASES = [(3, True), (3, False), (4, True), (4, False)]
SEED = {"concat": 31, "max-pool": 36, "attn": 31}      # 36: the gap condition below holds (31-35 do not all)
MAX_GAP = 1e-4          # smallest allowed gap between the two largest h_t of an element, relative to max|h|


def batch():
    store = synth.make_store(6, seed=23, n_lo=2, n_hi=12, n_mean=6)
    # one molecule with an isolated atom (no bond at all): a real row of its own in the packed layout, not padding
    store.append(synth.Molecule(np.array([6, 8, 7, 6], np.int32), np.array([[0, 1, 0], [1, 2, 1]], np.int32)))
    return synth.concat_mols(store)


def max_gap(h_list):
    x = torch.stack(h_list).detach()
    top = x.topk(2, dim=0).values
    return float((top[0] - top[1]).min() / x.abs().max())


def build(aggregator):
    atoms, adj = batch()
    out = {"atoms": atoms, "adj": adj}
    ta, tj = torch.from_numpy(atoms), torch.from_numpy(adj).double()
    for T, tied in CASES:
        tag = f"c{T}{'t' if tied else 'u'}"
        p = AR.make_agg_params(SEED[aggregator] + 7 * T + int(tied), D, OUT, T, aggregator, weight_tying=tied,
                               n_atom_types=N_ATOM_TYPES)
        p = {k: v.float().double().requires_grad_() for k, v in p.items()}
        gw = torch.from_numpy(np.random.RandomState(5 + T).normal(size=(atoms.shape[0], OUT)))
        g, h_list = AR.ggnn_agg_forward(p, ta, tj, T, aggregator, weight_tying=tied)
        if aggregator == "max-pool":
            gap = max_gap(h_list)
            assert gap >= MAX_GAP, f"{tag}: two layers within {gap:.2e} of max|h| of each other; pick another seed"
            out[f"{tag}:gap"] = np.asarray(gap)
        grads = torch.autograd.grad((g * gw).sum(), list(p.values()))
        h0 = p["embed/W"].detach()[ta.long()].requires_grad_()
        g2, _ = AR.ggnn_agg_forward(p, h0, tj, T, aggregator, weight_tying=tied)
        (dh0,) = torch.autograd.grad((g2 * gw).sum(), [h0])
        out[f"{tag}:g"], out[f"{tag}:gw"], out[f"{tag}:dh0"] = g.detach().numpy(), gw.numpy(), dh0.numpy()
        for (k, v), dv in zip(p.items(), grads):
            out[f"{tag}:p:{k}"], out[f"{tag}:d:{k}"] = v.detach().numpy().astype(np.float32), dv.numpy().astype(np.float32)
    return out


if __name__ == "__main__":
    for agg, name in FILES.items():
        np.savez_compressed(os.path.join(HERE, name), **build(agg))
