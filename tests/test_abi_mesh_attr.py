"""include/pvd_hip_mesh_attr.h -- per-vertex normals of the extracted mesh -- next to include/pvd_hip_mesh.h: the new header declares
exactly one name, libpvd_hip.so exports it, the binding lists it in a tuple of its own, and the other headers, their lists and the ABI
number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OTHERS = ("pvd_hip.h", "pvd_hip_mlp.h", "pvd_hip_metrics.h", "pvd_hip_data.h", "pvd_hip_march.h", "pvd_hip_mesh.h", "pvd_hip_components.h")


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_header_declares_exactly_the_one_entry_point():
    assert _declared("pvd_hip_mesh_attr.h") == ["pvd_mesh_normals"]
    src = _source("pvd_hip_mesh_attr.h")
    assert '#include "pvd_hip.h"' in src
    assert "utils.py:442-488" in src


def test_the_library_exports_it_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    assert hasattr(lib, "pvd_mesh_normals"), "libpvd_hip.so does not export pvd_mesh_normals"
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh.h") == ["pvd_mesh_count", "pvd_mesh_emit", "pvd_mesh_workspace_bytes"]
    for h in OTHERS:
        assert "pvd_mesh_normals" not in _declared(h), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_it_in_a_tuple_of_its_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_ATTR, tuple)
    assert sorted(pvd_hip.ENTRY_POINTS_MESH_ATTR) == _declared("pvd_hip_mesh_attr.h")
    assert sorted(pvd_hip.ENTRY_POINTS_MESH) == _declared("pvd_hip_mesh.h")
    assert sorted(pvd_hip.ENTRY_POINTS) == _declared("pvd_hip.h")
    assert not set(pvd_hip.ENTRY_POINTS_MESH_ATTR) & set(pvd_hip.ENTRY_POINTS + pvd_hip.ENTRY_POINTS_MLP + pvd_hip.ENTRY_POINTS_METRICS
                                                         + pvd_hip.ENTRY_POINTS_DATA + pvd_hip.ENTRY_POINTS_MARCH + pvd_hip.ENTRY_POINTS_MESH
                                                         + pvd_hip.ENTRY_POINTS_COMPONENTS)
    assert callable(pvd_hip.mesh_normals)
    assert pvd_hip.ABI_VERSION == 6


def test_the_binding_rejects_cpu_tensors(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    R = 4
    field, ws = torch.zeros(R, R, R), torch.zeros(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_normals(field, R, 0.0, torch.zeros(3), torch.ones(3), ws, torch.zeros(1, 3))


def test_the_entry_point_checks_its_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, an unaligned or short workspace: PVD_ERR_INVALID; R outside 2..512: PVD_ERR_UNSUPPORTED; no vertices: PVD_OK --
    all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp, sz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    one = vp(16)  # a non-NULL value that is never dereferenced on these paths
    size = lib.pvd_mesh_workspace_bytes
    size.restype = ctypes.c_size_t
    lib.pvd_mesh_normals.restype = ctypes.c_int

    def normals(field=one, R=8, bmin=one, bmax=one, ws=one, nbytes=None, out=one, V=0):
        return lib.pvd_mesh_normals(field, u32(R), f32(0.5), bmin, bmax, ws, sz(size(u32(R)) if nbytes is None else nbytes), out, u32(V),
                                    vp(0))
    assert normals() == 0 and normals(out=vp(0)) == 0  # V == 0: nothing to do
    assert normals(field=vp(0)) == -1 and normals(bmin=vp(0)) == -1 and normals(bmax=vp(0)) == -1 and normals(ws=vp(0)) == -1
    assert normals(nbytes=size(u32(8)) - 1) == -1 and normals(nbytes=0) == -1 and normals(ws=vp(18)) == -1
    assert normals(out=vp(0), V=3) == -1
    assert normals(R=0, nbytes=1 << 40) == -2 and normals(R=1, nbytes=1 << 40) == -2 and normals(R=513, nbytes=1 << 40) == -2
    assert normals(R=513, nbytes=1 << 40, V=3) == -2 and normals(field=vp(0), V=3) == -1  # with vertices too: the checks come first
