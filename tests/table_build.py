"""What the CPU checks of the tile-table families share (tests/test_ggate_enc_build.py, test_ggdev_enc_build.py,
test_jk_table_build.py, test_gin_table_build.py, test_rows_entry.py): the built library, a C entry's argument list from the header,
the table entries' argument-list rule, the bad-table cases of the argument checks, a translation unit's kernel resource usage and
a small encoder-layout batch.  No GPU is needed."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcn-bmp_amd", "csrc")


def lib():
    """bmp._lib with the library built."""
    import __graft_entry__ as g
    g.build()
    from bmp import _lib
    return _lib


def header_args(name):
    src = open(os.path.join(ROOT, "include", "bmp.h")).read()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def check_table_entries(names, whole_of=lambda name: name.replace("_table", "_tile")):
    """Each table entry is declared in the header and the ctypes table with one ctypes entry per argument, and its list is the
    whole-tile entry's, then the table: mt_row0, mt_nblk, mt_rows, tile_stride in front of the stream."""
    _l = lib()
    for name in names:
        args, whole = header_args(name), header_args(whole_of(name))
        assert name in _l.SIGNATURES, name
        assert len(args) == len(_l.SIGNATURES[name][1]), (name, len(args), len(_l.SIGNATURES[name][1]))
        assert args[:len(whole) - 1] == whole[:-1] and args[-1] == whole[-1], name
        assert [a.split()[-1].lstrip("*") for a in args[len(whole) - 1:-1]] == ["mt_row0", "mt_nblk", "mt_rows", "tile_stride"], name
        assert _l.SIGNATURES[name][1][:len(whole) - 1] == _l.SIGNATURES[whole_of(name)][1][:-1]
        assert hasattr(_l.lib(), name), name


# A non-null, 16-byte aligned address nobody reads: every case built from it fails an argument check, which returns before any
# launch.
P = 0x10000
BAD_TABLES = [dict(r0=None), dict(nb=None), dict(rows=0), dict(stride=96), dict(stride=130)]
bad_id = lambda b: "-".join(f"{k}={v}" for k, v in b.items())


def resource_usage(src, tmp, *flags):
    """(kernel names, scratch bytes per lane, VGPRs, AGPRs, waves per SIMD, LDS bytes per block) of one translation unit."""
    import __graft_entry__ as g
    r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", CSRC, *flags,
                        "-c", os.path.join(CSRC, src), "-o", os.path.join(tmp, src + ".o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    grab = lambda pat: [int(x) for x in re.findall(pat, r.stderr)]
    return (re.findall(r"Function Name: (\S+)", r.stderr), grab(r"ScratchSize \[bytes/lane\]: (\d+)"), grab(r" VGPRs: (\d+)"),
            grab(r" AGPRs: (\d+)"), grab(r"Occupancy \[waves/SIMD\]: (\d+)"), grab(r"LDS Size \[bytes/block\]: (\d+)"))


def enc_batch():
    """Six small molecules, three pairs, in the encoder layout with dedup, on the host."""
    from bmp import enclayout, packed, synth
    store = synth.make_store(6, seed=2, n_lo=2, n_hi=20, n_mean=8)
    return enclayout.encode_from_store(packed.MolStore(store), [np.array([0, 1, 2]), np.array([3, 4, 0])], dedup=True)
