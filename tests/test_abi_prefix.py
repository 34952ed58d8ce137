"""include/pvd_hip_prefix.h -- the prefix of a group of G steps in one launch per stage -- next to include/pvd_hip.h: the header declares
exactly four names, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the entry points check their
arguments before any launch (no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_composite_rays_train_bg_forward_group", "pvd_make_ray_batch_group", "pvd_march_group_workspace_bytes", "pvd_march_rays_train_group"]


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_header_declares_exactly_the_four_entry_points():
    assert _declared("pvd_hip_prefix.h") == NAMES


def test_the_library_exports_them_and_the_binding_lists_them(hip_lib_built):
    import pvd_hip
    lib = ctypes.CDLL(hip_lib_built)
    for s in NAMES:
        assert hasattr(lib, s), "libpvd_hip.so does not export %s" % s
    assert sorted(pvd_hip.ENTRY_POINTS_PREFIX) == NAMES
    assert not set(pvd_hip.ENTRY_POINTS_PREFIX) & set(pvd_hip.ENTRY_POINTS + pvd_hip.ENTRY_POINTS_MARCH)
    lib.pvd_march_group_workspace_bytes.restype = ctypes.c_size_t
    lib.pvd_march_workspace_bytes.restype = ctypes.c_size_t
    u32 = ctypes.c_uint32
    assert lib.pvd_march_group_workspace_bytes(u32(64), u32(257)) == 257 * lib.pvd_march_workspace_bytes(u32(64)) == 257 * 65 * 256


def test_the_march_entry_checks_its_arguments_before_any_launch(hip_lib_built):
    """No workspace, a workspace that is too small, a segment beyond 16384 rays and more segments than a grid has rows are
    PVD_ERR_INVALID before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp, sz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    one, null = vp(256), vp(0)

    def call(N, G, ws, ws_bytes):
        return lib.pvd_march_rays_train_group(one, one, one, f32(1.0), f32(0.0), u32(1024), u32(N), u32(G), u32(1), u32(128), u32(256), one, one, one,
                                              one, one, one, one, u32(1), ws, sz(ws_bytes), u32(1), null, u32(0), null, null)
    assert call(64, 3, null, 0) == -1
    assert call(64, 3, one, 3 * 65 * 256 - 1) == -1
    assert call(16385, 1, one, 1 << 40) == -1
    assert call(64, 65536, one, 1 << 40) == -1
    assert call(64, 0, null, 0) == 0
