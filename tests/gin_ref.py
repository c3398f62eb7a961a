"""Dense restatement of the graph isomorphism network encoder (the reference's models/gin.py), op for op, in the dtype of the
parameters it is given (float64 for reference values, float32 for the error estimate of the relu kink condition below).

    h0 = h = embed[atoms]                                         (mb, A, d)
    adjsum = adj.sum(axis=1)                                      (mb, A, A): bond types summed, entries with their values
    per layer that RUNS:  s = adjsum @ h + h;  t = relu(s W1^T + b1);  h = relu(keep * (t W2^T + b2))
                          concat_hidden: g_list += readout_step([h, h0])
    readout([h, h0]) = act(sum over ALL A positions (times is_real_node) of sigmoid(x Wi^T + bi) * act(x Wj^T + bj))
    the loop runs range(n_message_layers): ONE layer when the weights are tied, n_layers layers when they are not.
Nothing is masked by position: padded positions (id 0, no bonds) count everywhere.

Parameter names are the link paths of the reference: embed/W, update_layers/{i}/linear_g{1,2}/{W,b},
readout_layers/{k}/{i,j}_layer/{W,b}; Linear weights are [out x in], the readout's input is [h, h0] (2 d wide).

RELU KINK CONDITION.  A float32 result and the float64 reference can disagree about the sign of a pre-activation that is
nearly zero, which flips a whole gradient contribution.  Every gradient case of tests/test_gpu_gin.py therefore takes its
(seed, shape, data) from KINK_TABLE, whose seeds were searched on the CPU (``python tests/gin_ref.py`` prints the table) so
that the float64 restatement's smallest |pre-activation| over every linear of every layer that runs (elements a given dropout
mask zeroes excluded: both sides multiply them by an exact 0) is at least 8 x the largest |pre32 - pre64| of this restatement
evaluated in float32 on the CPU.  The margin is measured on the reference alone; the factor 8 covers a summation order that
differs from torch's.  tests/test_gin_ref.py asserts the condition for every row.
"""
import math

import numpy as np
import torch

ACTS = {"identity": lambda x: x, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu}
KINK_FACTOR = 8.0


def make_gin_params(seed, hidden, out, layers, tying, concat_hidden=False, n_atom_types=117, dtype=torch.float64, prefix="",
                    bias=0.3):
    """Fixed draw order: embed, the update layers (W1, b1, W2, b2 each), then the readout layers (Wi, bi, Wj, bj each): the
    encoder states of a seed do not depend on ``concat_hidden``."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    p = {prefix + "embed/W": r(n_atom_types, hidden)}
    for i in range(1 if tying else layers):
        for k in (1, 2):
            p[f"{prefix}update_layers/{i}/linear_g{k}/W"] = r(hidden, hidden) / math.sqrt(hidden)
            p[f"{prefix}update_layers/{i}/linear_g{k}/b"] = bias * r(hidden)
    for k in range(layers if concat_hidden else 1):
        for n in ("i", "j"):
            p[f"{prefix}readout_layers/{k}/{n}_layer/W"] = r(out, 2 * hidden) / math.sqrt(2 * hidden)
            p[f"{prefix}readout_layers/{k}/{n}_layer/b"] = bias * r(out)
    return {k: v.to(dtype) for k, v in p.items()}


def gin_forward(params, atoms, adj, tying=True, concat_hidden=False, keep=None, is_real_node=None, activation="identity",
                prefix="", pre=None):
    """(g, h).  ``keep``: one (mb, A, d) mask per layer that runs (values 0 or 1 / (1 - p)), or None.  ``pre`` (a list):
    receives every pre-activation, the second linear's with its mask's zeros set to NaN."""
    p = params
    dt = p[prefix + "embed/W"].dtype
    n_msg = 1 + max(int(k[len(prefix):].split("/")[1]) for k in p if k.startswith(prefix + "update_layers/"))
    assert not tying or n_msg == 1
    act = ACTS[activation]
    atoms = torch.as_tensor(np.asarray(atoms)).long()
    adjsum = torch.as_tensor(np.asarray(adj)).to(dt).sum(dim=1)
    real = None if is_real_node is None else torch.as_tensor(np.asarray(is_real_node)).to(dt)

    def readout(k, h, h0):
        x = torch.cat((h, h0), dim=2)
        q = f"{prefix}readout_layers/{k}/"
        gi = torch.sigmoid(x @ p[q + "i_layer/W"].t() + p[q + "i_layer/b"])
        gj = act(x @ p[q + "j_layer/W"].t() + p[q + "j_layer/b"])
        gg = gi * gj
        if real is not None:
            gg = gg * real[:, :, None]
        return act(gg.sum(dim=1))

    h = p[prefix + "embed/W"][atoms]
    h0 = h
    g_list = []
    for step in range(n_msg):                                   # models/gin.py:215
        q = f"{prefix}update_layers/{0 if tying else step}/"
        s = adjsum @ h + h
        p1 = s @ p[q + "linear_g1/W"].t() + p[q + "linear_g1/b"]
        t = torch.relu(p1)
        p2 = t @ p[q + "linear_g2/W"].t() + p[q + "linear_g2/b"]
        if pre is not None:
            pre.append(p1.detach())
        if keep is not None:
            k_ = keep[step].to(dt)
            if pre is not None:
                pre.append(torch.where(k_ != 0, p2.detach(), torch.full_like(p2, float("nan"))))
            p2 = p2 * k_
        elif pre is not None:
            pre.append(p2.detach())
        h = torch.relu(p2)
        if concat_hidden:
            g_list.append(readout(step, h, h0))
    if concat_hidden:
        return torch.cat(g_list, dim=1), h
    return readout(0, h, h0), h


# ---------------------------------------------------------------------------------------------------------
# the data sets of the GPU tests (seeded; built once per process) and the table of (seed, shape, data) rows
# ---------------------------------------------------------------------------------------------------------
_DATA = {}


def data(name):
    """dict(sides=[(atoms (mb, A) int32, adj (mb, 4, A, A) float32), ...], and, for data packed from a store, store / idx / pb
    (a host PackedMolBatch with its dense maps))."""
    if name in _DATA:
        return _DATA[name]
    from bmp import packed, synth
    if name == "fixture":                      # the 40-molecule store, 13 + 13 instances (as tests/test_gpu_nfp.py)
        store = synth.make_store(40, seed=9, n_lo=2, n_hi=30, n_mean=10)
        rs = np.random.RandomState(2)
        idx = [rs.randint(0, 40, 13), rs.randint(0, 40, 13)]
    elif name == "oversized":                  # one molecule of 150 atoms (it spans two tiles) beside three small ones
        store = synth.make_store(3, seed=4, n_lo=3, n_hi=12, n_mean=6) + synth.make_store(1, seed=6, n_lo=150, n_hi=150, n_mean=150)
        idx = [np.array([0, 3, 1, 2])]
    elif name == "small":                      # five small molecules, one side: the dense call form, is_real_node
        store = synth.make_store(5, seed=21, n_lo=2, n_hi=12, n_mean=6)
        idx = [np.arange(5)]
    else:
        raise KeyError(name)
    pb = packed.pack_from_store(packed.MolStore(store), idx, device="cpu", with_dense_map=True)
    sides = [synth.concat_mols([store[k] for k in ix]) for ix in idx]
    _DATA[name] = dict(store=store, idx=idx, pb=pb, sides=sides)
    return _DATA[name]


def keep_rows(name, hidden, steps, p, seed):
    """``steps`` dropout masks on the packed rows of data set ``name`` ((n_rows, hidden) float32, values 0 or 1 / (1 - p)): the
    pad row of a molecule carries one mask for all its padded positions."""
    g = torch.Generator().manual_seed(seed)
    n = data(name)["pb"].n_rows
    return [(torch.rand(n, hidden, generator=g) >= p).float() * (1.0 / (1.0 - p)) for _ in range(steps)]


def keep_dense(name, rows, side):
    """The row masks at the dense positions of one side: [(mb, A, hidden)] per step."""
    dm = data(name)["pb"].dense_maps[side]
    return [k[dm] for k in rows]


# name: seed, hidden, out, layers, tying, data, (dropout p, mask seed) or None.  Beside each row the measured
# min |pre64| / max |pre32 - pre64| = margin, as printed by ``python tests/gin_ref.py`` (which searches the seeds: the first
# seed >= 1 that meets the factor of 8)
KINK_TABLE = {
    "c16": dict(seed=1, hidden=16, out=16, layers=2, tying=False, data="fixture", drop=None),           # 3.4e-4 / 3.1e-6 = 110 x
    "c24": dict(seed=1, hidden=24, out=12, layers=4, tying=True, data="fixture", drop=None),            # 4.9e-4 / 1.4e-6 = 363 x
    "f64": dict(seed=1, hidden=64, out=32, layers=3, tying=False, data="fixture", drop=None),           # 3.9e-4 / 1.6e-5 = 24 x
    "f128": dict(seed=2, hidden=128, out=128, layers=2, tying=False, data="fixture", drop=None),        # 8.8e-5 / 7.5e-6 = 11.7 x
    "over16": dict(seed=1, hidden=16, out=8, layers=2, tying=False, data="oversized", drop=None),       # 3.6e-4 / 3.4e-6 = 105 x
    "over64": dict(seed=1, hidden=64, out=16, layers=2, tying=False, data="oversized", drop=None),      # 2.8e-4 / 1.2e-5 = 22.5 x
    "small64": dict(seed=1, hidden=64, out=16, layers=2, tying=False, data="small", drop=None),         # 1.6e-4 / 4.7e-6 = 33 x
    "small16": dict(seed=1, hidden=16, out=8, layers=2, tying=False, data="small", drop=None),          # 1.7e-3 / 2.5e-6 = 687 x
    "keep64": dict(seed=2, hidden=64, out=16, layers=2, tying=False, data="fixture", drop=(0.5, 11)),   # 1.7e-4 / 7.1e-6 = 24 x
    "keep16": dict(seed=1, hidden=16, out=8, layers=2, tying=False, data="fixture", drop=(0.5, 12)),    # 3.6e-4 / 4.0e-6 = 90 x
    "pair16": dict(seed=1, hidden=16, out=16, layers=2, tying=True, data="fixture", drop=(0.5, 13)),    # 3.6e-4 / 1.1e-6 = 318 x
}


def row_keep(row):
    """The row's masks on the packed rows (None without dropout)."""
    if row["drop"] is None:
        return None
    steps = 1 if row["tying"] else row["layers"]
    return keep_rows(row["data"], row["hidden"], steps, row["drop"][0], row["drop"][1])


def row_params(row, concat_hidden=False, prefix=""):
    return make_gin_params(row["seed"], row["hidden"], row["out"], row["layers"], row["tying"], concat_hidden, prefix=prefix)


def kink_margin(row):
    """(min |pre64|, max |pre32 - pre64|) of a table row over all its sides."""
    d = data(row["data"])
    p64 = row_params(row)
    p32 = {k: v.float() for k, v in p64.items()}
    kr = row_keep(row)
    lo, err = float("inf"), 0.0
    for side, (atoms, adj) in enumerate(d["sides"]):
        kd = None if kr is None else keep_dense(row["data"], kr, side)
        a, b = [], []
        with torch.no_grad():
            gin_forward(p64, atoms, adj, row["tying"], keep=kd, pre=a)
            gin_forward(p32, atoms, adj, row["tying"], keep=kd, pre=b)
        for x, y in zip(a, b):
            live = ~torch.isnan(x)
            lo = min(lo, x[live].abs().min().item())
            err = max(err, (y.double()[live] - x[live]).abs().max().item())
    return lo, err


def kink_ok(row):
    lo, err = kink_margin(row)
    return lo >= KINK_FACTOR * err


def search_seed(row, start=1, stop=4000):
    for seed in range(start, stop):
        r = dict(row, seed=seed)
        if kink_ok(r):
            return seed
    raise RuntimeError("no seed found")


if __name__ == "__main__":
    import os
    import sys
    HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "gcn-bmp_amd")]
    for name, row in KINK_TABLE.items():
        seed = search_seed(row)
        lo, err = kink_margin(dict(row, seed=seed))
        print(f'"{name}": seed={seed}  min|pre64| {lo:.3e}  max|pre32-pre64| {err:.3e}  margin {lo / err:.1f}x')
