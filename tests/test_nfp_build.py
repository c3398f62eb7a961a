"""Compile-time condition of the NFP kernels: zero scratch for the fused tile kernels (and every other kernel of
csrc/bmp_nfp.hip), read from the compiler's resource report for gfx950.  No GPU needed."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nfp_kernels_have_no_scratch():
    import __graft_entry__ as g
    csrc = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", csrc, "-c",
                            os.path.join(csrc, "bmp_nfp.hip"), "-o", os.path.join(tmp, "nfp.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) and len(names) >= 18
    tile = [n for n in names if "k_nfp_tile_fwd" in n or "k_nfp_tile_bwd" in n or "k_nfp_readout_tile" in n]
    assert len(tile) == 8, tile                                        # fwd, bwd, readout fwd, readout bwd at d = 64 and 128
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
