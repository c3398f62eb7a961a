"""Compile-time condition of the NFP kernels: zero scratch for the fused tile kernels (and every other kernel of
csrc/bmp_nfp.hip, and the row-list kernels of csrc/bmp_graph.hip that build its rows by degree class), read from the
compiler's resource report for gfx950.  No GPU needed."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(g, csrc, tmp, name):
    return subprocess.Popen([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                             os.path.join(csrc, name + ".hip"), "-o", os.path.join(tmp, name + ".o"),
                             "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _scratch(proc):
    err = proc.communicate()[1]
    assert proc.returncode == 0, err[-2000:]
    names = re.findall(r"Function Name: (\S+)", err)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    assert len(names) == len(scratch)
    return names, scratch


def test_nfp_kernels_have_no_scratch():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        procs = [_report(g, csrc, tmp, n) for n in ("bmp_nfp", "bmp_graph")]
        (names, scratch), (gnames, gscratch) = [_scratch(p) for p in procs]
    assert len(names) >= 16
    tile = [n for n in names if "k_nfp_tile_fwd" in n or "k_nfp_tile_bwd" in n or "k_nfp_readout_tile" in n]
    assert len(tile) == 8, tile                                        # fwd, bwd, readout fwd, readout bwd at d = 64 and 128
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    # the rows-by-degree-class kernels are instances of the row-list builder of bmp_graph.hip (count and emit: 4, 5, 7 lists)
    lists = {n: s for n, s in zip(gnames, gscratch) if "k_row_lists" in n}
    assert len(lists) == 6 and all(s == 0 for s in lists.values()), lists
