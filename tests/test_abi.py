"""The C-ABI library loads without a GPU and exports every symbol include/captra_hip.h declares;
the product path refuses to run on CPU tensors instead of falling back."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def declared_symbols():
    text = (ROOT / "include" / "captra_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(captra_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_ten_pointnet2_ops():
    syms = declared_symbols()
    for name in ("captra_ball_query", "captra_group_points", "captra_group_points_grad", "captra_gather_points",
                 "captra_gather_points_grad", "captra_furthest_point_sampling", "captra_knn", "captra_three_nn",
                 "captra_three_interpolate", "captra_three_interpolate_grad"):
        assert name in syms


def test_library_exports_every_declared_symbol():
    from captra_amd import _lib
    assert _lib.LIB_PATH.exists(), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"declared in captra_hip.h but not exported: {missing}"
    lib.captra_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.captra_version()


def test_python_binding_table_matches_header():
    from captra_amd import _lib
    syms = set(declared_symbols())
    for name in list(_lib._SIGNATURES) + list(_lib._AUX_SIGNATURES):
        assert name in syms, f"{name} bound in _lib.py but not declared in the header"
    assert not set(_lib._SIGNATURES) & set(_lib._AUX_SIGNATURES)
    for name in _lib.EX_ENTRY_POINTS:
        assert name in _lib._SIGNATURES and name + "_ex" in syms


def test_launch_plumbing_lives_in_common_h():
    """Per-device kernel attributes, the CU count and the occupancy query are common.h / prof.cpp's (captra_allow_lds,
    captra_device_cus, captra_free_cus, captra_blocks_per_cu): no kernel family carries a copy of its own."""
    csrc = ROOT / "captra_amd" / "csrc"
    banned = ("hipFuncSetAttribute", "hipGetDeviceProperties", "hipOccupancyMaxActiveBlocksPerMultiprocessor", "CaptraDeviceOnce",
              "hipDeviceGetAttribute")
    hips = sorted(csrc.glob("*.hip"))
    assert hips
    bad = [(p.name, word) for p in hips for word in banned if word in p.read_text()]
    assert not bad, bad
    others = [p.name for p in sorted(csrc.iterdir()) if p.suffix in (".h", ".cpp") and p.name not in ("common.h", "prof.cpp")
              and "hipDeviceGetAttribute" in p.read_text()]
    assert not others, others


def test_cross_lane_primitives_live_in_wave_ops_h():
    """DPP moves, the xor-butterfly accumulation and the workgroup sum are csrc/wave_ops.h's: no kernel family carries a copy."""
    csrc = ROOT / "captra_amd" / "csrc"
    files = [p for p in sorted(csrc.iterdir()) if p.suffix in (".hip", ".h", ".cpp")]
    assert (csrc / "wave_ops.h") in files
    texts = {p.name: p.read_text() for p in files}
    for word in ("__builtin_amdgcn_update_dpp", "+= __shfl_xor("):
        holders = [name for name, text in texts.items() if word in text and name != "wave_ops.h"]
        assert not holders, (word, holders)
    assert "__builtin_amdgcn_update_dpp" in texts["wave_ops.h"]
    removed = ("fp_dpp_max", "dpp_f<", "sp_dpp<", "sw_dpp_sel<", "block_reduce_sum", "rs_block_sum")
    bad = [(name, word) for name, text in texts.items() for word in removed if word in text]
    assert not bad, bad


def test_pointnet2_cuda_module_surface():
    """Same ten callables as the reference's pybind module (pointnet2_api.cpp:10-25)."""
    import captra_amd
    from captra_amd import pointnet2_cuda
    for name in ("ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper", "gather_points_wrapper",
                 "gather_points_grad_wrapper", "furthest_point_sampling_wrapper", "knn_wrapper", "three_nn_wrapper",
                 "three_interpolate_wrapper", "three_interpolate_grad_wrapper"):
        assert callable(getattr(pointnet2_cuda, name))
    captra_amd.install_as_pointnet2_cuda()
    import pointnet2_cuda as alias
    assert alias is pointnet2_cuda


def test_no_cpu_fallback():
    from captra_amd.pointnet_lib import pointnet2_utils as pn
    with pytest.raises(RuntimeError):
        pn.furthest_point_sample(torch.zeros(1, 16, 3), 4)
    with pytest.raises(RuntimeError):
        pn.ball_query(0.1, 4, torch.zeros(1, 16, 3), torch.zeros(1, 2, 3))


def test_product_code_never_imports_the_oracle():
    bad = []
    for path in (ROOT / "captra_amd").rglob("*.py"):
        text = path.read_text()
        if re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M) or "libcaptra_oracle" in text.replace("libcaptra_oracle.so\"", ""):
            if path.name != "build.py":
                bad.append(str(path))
    assert not bad, bad
