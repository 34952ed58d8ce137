"""include/pvd_hip_march.h -- the coarse occupancy mask and the training marcher that takes it -- next to include/pvd_hip.h: the new
header declares exactly two names, libpvd_hip.so exports them, the binding lists them in a tuple of their own, apart from every other
header's names (what pvd_hip.h holds and the ABI number are pinned once, in tests/test_abi_symbols.py; no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OTHER_HEADERS = ("pvd_hip.h", "pvd_hip_mlp.h", "pvd_hip_metrics.h", "pvd_hip_data.h")


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_march_header_declares_exactly_the_two_entry_points():
    assert _declared("pvd_hip_march.h") == ["pvd_march_rays_train_mask", "pvd_occ_coarse_mask"]
    assert '#include "pvd_hip.h"' in _source("pvd_hip_march.h")


def test_the_library_exports_them_apart_from_the_other_headers(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for s in _declared("pvd_hip_march.h"):
        assert hasattr(lib, s), "libpvd_hip.so does not export %s" % s
    for h in OTHER_HEADERS:
        assert not set(_declared(h)) & set(_declared("pvd_hip_march.h")), h


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert sorted(pvd_hip.ENTRY_POINTS_MARCH) == _declared("pvd_hip_march.h")
    assert not set(pvd_hip.ENTRY_POINTS_MARCH) & set(pvd_hip.ENTRY_POINTS)
    assert callable(pvd_hip.occ_coarse_mask)
    assert pvd_hip.COARSE_BLOCK == int(re.search(r"#define PVD_COARSE_BLOCK (\d+)", _source("pvd_hip_march.h")).group(1)) == 8
    assert pvd_hip.coarse_mask_bytes(1, 128) == 4096 and pvd_hip.coarse_mask_bytes(2, 64) == 1024 and pvd_hip.coarse_mask_bytes(1, 100) == 0 and pvd_hip.coarse_mask_bytes(1, 24) == 0 and pvd_hip.coarse_mask_bytes(3, 8) == 3


def test_the_mask_entry_checks_its_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, C or H out of range and a misaligned bitfield are PVD_ERR_INVALID, an H that is no power of two >= 8
    PVD_ERR_UNSUPPORTED -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    one, null = vp(256), vp(0)
    assert lib.pvd_occ_coarse_mask(null, u32(1), u32(128), one, null) == -1
    assert lib.pvd_occ_coarse_mask(one, u32(1), u32(128), null, null) == -1
    assert lib.pvd_occ_coarse_mask(one, u32(0), u32(128), one, null) == -1 and lib.pvd_occ_coarse_mask(one, u32(17), u32(128), one, null) == -1
    assert lib.pvd_occ_coarse_mask(one, u32(1), u32(0), one, null) == -1 and lib.pvd_occ_coarse_mask(one, u32(1), u32(2048), one, null) == -1
    assert lib.pvd_occ_coarse_mask(vp(264), u32(1), u32(128), one, null) == -1
    for h in (100, 24, 96, 4):  # (24, 96: multiples of 8 whose Morton order leaves the cascade)
        assert lib.pvd_occ_coarse_mask(one, u32(1), u32(h), one, null) == -2, h
