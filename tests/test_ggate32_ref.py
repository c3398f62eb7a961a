"""CPU checks of the hidden-width-32 cases of the gated GGNN encoders (tests/ggate32_ref.py): the float32 restatement of every
case stays inside parity_util.close (max-norm 1e-4) of the float64 one -- so the bound the GPU tests apply is one a float32
implementation can meet on these inputs, relu kinks of the pair model's link predictor included -- and the data set "blocks"
has the four 32-row blocks it is built for.  No GPU."""
import pytest
import torch

import ggate32_ref as R


def close(got, want, name, tol=1e-4, floor=1e-6):
    """parity_util.close's comparison (max |got - want| <= tol * max |want|) without its log: a CPU session leaves the GPU
    sessions' achieved-error log alone."""
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, name
    rel = ((got - want).abs().max().item() if got.numel() else 0.0) / max(want.abs().max().item(), floor)
    assert torch.isfinite(got).all() and rel <= tol, f"{name}: rel err {rel:.3e} > {tol:.0e}"
    return rel


def _worst(a, b, tag):
    w = [close(a["g"], b["g"], tag + " g")]
    w += [close(x, y, f"{tag} atoms {s + 1}") for s, (x, y) in enumerate(zip(a["atoms"], b["atoms"]))]
    for k, v in b["p"].items():
        if v.grad is None:           # (a link the file constructs and never calls)
            assert a["p"][k].grad is None, k
            continue
        w.append(close(a["p"][k].grad, v.grad, f"{tag} grad {k}"))
    return max(w)


@pytest.mark.parametrize("name", [n for n in R.CASES if n != R.PAIR_CASE])
def test_float32_restatement_is_inside_the_bound(name):
    keep_seed = 11 if name == "fuse_keep32" else None
    r64 = R.reference(name, keep_seed=keep_seed)
    r32 = R.reference(name, keep_seed=keep_seed, dtype=torch.float32)
    assert all(v.dtype == torch.float32 for v in r32["p"].values()) and r32["g"].dtype == torch.float32
    print(f"[ggate32] {name}: float32 vs float64 worst rel {_worst(r32, r64, name):.1e}")


def test_pair_model_float32_restatement_is_inside_the_bound():
    r64, r32 = R.pair_reference(), R.pair_reference(torch.float32)
    w = [close(r32["y"], r64["y"], "pair logits"), close(r32["loss"], r64["loss"], "pair loss")]
    w += [close(r32["grads"][k], v, f"pair grad {k}") for k, v in r64["grads"].items()]
    # no relu of the link predictor sits closer to its kink than the float32 restatement's error there
    lo = min(a.abs().min().item() for a in r64["pre"])
    err = max((a.double() - b).abs().max().item() for a, b in zip(r32["pre"], r64["pre"]))
    print(f"[ggate32] pair: float32 vs float64 worst rel {max(w):.1e}; min |pre| {lo:.1e}, max |pre32 - pre64| {err:.1e}")
    assert lo > 8 * err


def test_blocks_property():
    pb = R.data("blocks")["pb"]
    assert pb.n_rows == 128 and pb.n_mols == 18
    got = R.block_types(pb)
    assert got[0] == ({1}, 32), got                 # one bond type only
    assert got[1] == ({0, 1, 2, 3}, 32), got        # all four
    assert got[2] == (set(), 32), got               # molecules (single atoms and their pad rows), no bond
    assert got[3] == (set(), 0), got                # fill past the last molecule
    assert R.block_types(pb, transposed=True) == got
    assert R.blocks_property(pb)
    assert not R.blocks_property(R.data("small")["pb"]) and not R.blocks_property(R.data("fixture")["pb"])


def test_dense_property():
    """More entries than the kernels stage in LDS, in both directions: the d = 32 kernels gather from the CSR in global memory."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcn-bmp_amd", "csrc", "bmp_tile.h")).read()
    assert int(re.search(r"#define FZ_ECAP (\d+)", src).group(1)) == R.STAGED_CSR_ENTRIES
    pb = R.data("dense")["pb"]
    assert pb.n_rows == 128 and pb.n_mols == 1 and int(pb.csr_ptr[128]) == int(pb.csrT_ptr[128]) == 1240
    assert set().union(*[t for t, _ in R.block_types(pb)]) == {0, 1, 2, 3}
    assert R.dense_property(pb)
    assert not R.dense_property(R.data("blocks")["pb"]) and not R.dense_property(R.data("fixture")["pb"])


def test_fixture_has_what_the_cases_count_on():
    pb = R.data("fixture")["pb"]
    assert pb.n_tiles == 3 and pb.n_mols == 26 and not pb.oversized
    types = set().union(*[t for t, _ in R.block_types(pb)])
    assert types == {0, 1, 2, 3}
    assert (pb.row_w > 1).any()                     # pad rows of multiplicity > 1
    assert R.data("oversized")["pb"].oversized
