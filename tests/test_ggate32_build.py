"""CPU checks of the hidden-width-32 gate step's surface: the C ABI's new symbols, the new source files, the kernels' resources
at the three-workgroups-per-CU design point, and the recorded model's constructor (RECORD.txt:404-405)."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gcn-bmp_amd", "csrc")
NEW = ("bmp_ggnn_gate_step_small_supported", "bmp_ggnn_gate_step_small_fwd", "bmp_ggnn_gate_step_small_bwd")


def test_new_symbols_in_header_and_ctypes_table():
    from bmp import _lib, functional as Fn
    src = open(os.path.join(ROOT, "include", "bmp.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    # the small entries take the argument lists of the two _tile_ entries
    assert _lib.SIGNATURES["bmp_ggnn_gate_step_small_fwd"] == _lib.SIGNATURES["bmp_ggnn_gate_step_tile_fwd"]
    assert _lib.SIGNATURES["bmp_ggnn_gate_step_small_bwd"] == _lib.SIGNATURES["bmp_ggnn_gate_step_tile_bwd"]
    assert Fn.GATE_PATHS.keys() == {"fused", "composed"}
    assert Fn.GATE_SMALL_DEFAULT.keys() == {"fuse", "gate"} and all(type(v) is bool for v in Fn.GATE_SMALL_DEFAULT.values())


def test_new_files_and_shared_helpers():
    gs = open(os.path.join(CSRC, "bmp_gate_small.hip")).read()
    fs = open(os.path.join(CSRC, "bmp_fused_small.hip")).read()
    st = open(os.path.join(CSRC, "bmp_stile.h")).read()
    assert '#include "bmp_stile.h"' in gs and '#include "bmp_stile.h"' in fs
    for name in ("fs_gather", "fs_wave_types", "fs_rm_buf", "fs_rm_ld", "fs_rm_st"):       # defined once, in the header
        pat = r"__device__ __forceinline__ \w+ %s\(" % name
        assert len(re.findall(pat, st)) == 1, name
        assert not re.search(pat, gs) and not re.search(pat, fs), name
    for name in ("FS_WSYNC", "FS_LOFF", "FS_FOR_ACC", "FS_R", "FS_NT"):
        pat = r"#define %s\b" % name
        assert len(re.findall(pat, st)) == 1 and not re.search(pat, gs) and not re.search(pat, fs), name
    # bmp_gate.hip keeps its eight kernels: the d = 32 instances live in the new file
    assert "bmp_ggnn_gate_step_small" not in open(os.path.join(CSRC, "bmp_gate.hip")).read()


def test_supported_widths():
    from bmp import functional as Fn
    assert [d for d in (8, 16, 24, 32, 40, 64, 128) if Fn.gate_step_small_supported(d)] == [32]
    assert [d for d in (8, 16, 24, 32, 40, 64, 128) if Fn.gate_step_supported(d)] == [64, 128]


def test_small_gate_kernels_fit_three_workgroups_per_cu():
    import __graft_entry__ as g
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([g._hipcc(), "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", CSRC, "-c",
                            os.path.join(CSRC, "bmp_gate_small.hip"), "-o", os.path.join(tmp, "gate_small.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    grab = lambda pat: [int(x) for x in re.findall(pat, r.stderr)]
    scratch = grab(r"ScratchSize \[bytes/lane\]: (\d+)")
    lds = grab(r"LDS Size \[bytes/block\]: (\d+)")
    occ = grab(r"Occupancy \[waves/SIMD\]: (\d+)")
    # two kinds x (forward saving, forward-only, backward)
    assert len(names) == len(scratch) == len(lds) == len(occ) == 6, names
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    # the launch's LDS request (gs_lds_bytes: two [128][36] tiles, the weighted degrees, the staged CSR) on top of the static part
    ecap = int(re.search(r"#define FZ_ECAP (\d+)", open(os.path.join(CSRC, "bmp_tile.h")).read()).group(1))
    dyn = (2 * 128 * 36 + 128 * 4 + 132 + 2 * ecap + 4) * 4
    src = open(os.path.join(CSRC, "bmp_gate_small.hip")).read()
    assert "(size_t)2 * FS_R * (D + 4) + FS_R * 4 + 132 + 2 * FZ_ECAP + 4) * sizeof(float)" in src
    assert all(s + dyn <= 160 * 1024 // 3 for s in lds), (dict(zip(names, lds)), dyn)
    assert all(o >= 3 for o in occ), dict(zip(names, occ))       # 4 waves per workgroup, one per SIMD: three workgroups per CU


def test_recorded_model_constructs_with_the_reference_parameter_names():
    """--fp-hidden-dim=32 --conv-layers=8 --weight-tying=False with the fuse-gate encoder."""
    import ggate32_ref as R
    from bmp.snapshot import param_dict
    from models.ggnn_dev_fuse import GGNN
    enc = GGNN(out_dim=16, hidden_dim=32, n_layers=8, weight_tying=False)
    want = R.make_params("fuse", 0, 32, 16, 8, False)
    got = param_dict(enc)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert tuple(got[k].shape) == tuple(v.shape), k
    assert enc.n_message_layer == 8 and tuple(enc.update_layer1.W.shape) == (32, 64)
