"""include/pvd_hip_mesh.h -- triangle meshes of a density volume -- next to include/pvd_hip.h: the new header declares exactly three
names, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the first header, its list and the ABI number
are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OTHERS = ("pvd_hip.h", "pvd_hip_mlp.h", "pvd_hip_metrics.h", "pvd_hip_data.h", "pvd_hip_march.h")


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_mesh_header_declares_exactly_the_three_entry_points():
    assert _declared("pvd_hip_mesh.h") == ["pvd_mesh_count", "pvd_mesh_emit", "pvd_mesh_workspace_bytes"]
    src = _source("pvd_hip_mesh.h")
    assert '#include "pvd_hip.h"' in src
    assert "utils.py:442-488" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    mine = set(_declared("pvd_hip_mesh.h"))
    for s in mine:
        assert hasattr(lib, s), "libpvd_hip.so does not export %s" % s
    assert len(_declared("pvd_hip.h")) == 75
    for h in OTHERS:
        assert not mine & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert sorted(pvd_hip.ENTRY_POINTS_MESH) == _declared("pvd_hip_mesh.h")
    assert sorted(pvd_hip.ENTRY_POINTS) == _declared("pvd_hip.h")
    assert not set(pvd_hip.ENTRY_POINTS_MESH) & set(pvd_hip.ENTRY_POINTS + pvd_hip.ENTRY_POINTS_MLP + pvd_hip.ENTRY_POINTS_METRICS
                                                    + pvd_hip.ENTRY_POINTS_DATA + pvd_hip.ENTRY_POINTS_MARCH)
    assert callable(pvd_hip.mesh_workspace_bytes) and callable(pvd_hip.mesh_count) and callable(pvd_hip.mesh_emit)
    assert pvd_hip.MESH_MAX_R == int(re.search(r"#define PVD_MESH_MAX_R (\d+)", _source("pvd_hip_mesh.h")).group(1)) == 512


def test_the_binding_rejects_cpu_tensors(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    R = 4
    field, ws = torch.zeros(R, R, R), torch.zeros(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_count(field, R, 0.0, ws, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_emit(field, R, 0.0, torch.zeros(3), torch.ones(3), ws, torch.zeros(1, 3), torch.zeros(1, 3, dtype=torch.int32))
    for bad in (0, 1, 513):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_workspace_bytes(bad)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, an unaligned or short workspace: PVD_ERR_INVALID; R outside 2..512: PVD_ERR_UNSUPPORTED; an emit of nothing:
    PVD_OK -- all before a device is touched (the pointers are never dereferenced); the workspace grows with R."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp, sz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    one = vp(16)  # a non-NULL value that is never dereferenced on these paths
    size = lib.pvd_mesh_workspace_bytes
    size.restype = ctypes.c_size_t
    lib.pvd_mesh_count.restype = lib.pvd_mesh_emit.restype = ctypes.c_int

    def count(field=one, R=8, ws=one, nbytes=None, totals=one):
        return lib.pvd_mesh_count(field, u32(R), f32(0.5), ws, sz(size(u32(R)) if nbytes is None else nbytes), totals, vp(0))

    def emit(field=one, R=8, bmin=one, bmax=one, ws=one, nbytes=None, verts=one, V=0, tris=one, T=0):
        return lib.pvd_mesh_emit(field, u32(R), f32(0.5), bmin, bmax, ws, sz(size(u32(R)) if nbytes is None else nbytes), verts, u32(V),
                                 tris, u32(T), vp(0))
    assert count(field=vp(0)) == -1 and count(ws=vp(0)) == -1 and count(totals=vp(0)) == -1
    assert count(nbytes=size(u32(8)) - 1) == -1 and count(nbytes=0) == -1 and count(ws=vp(18)) == -1
    assert count(R=0, nbytes=1 << 40) == -2 and count(R=1, nbytes=1 << 40) == -2 and count(R=513, nbytes=1 << 40) == -2

    assert emit() == 0 and emit(verts=vp(0), tris=vp(0)) == 0  # V == 0 and T == 0: nothing to do
    assert emit(field=vp(0)) == -1 and emit(bmin=vp(0)) == -1 and emit(bmax=vp(0)) == -1 and emit(ws=vp(0)) == -1
    assert emit(nbytes=size(u32(8)) - 1) == -1
    assert emit(verts=vp(0), V=3, T=1) == -1 and emit(tris=vp(0), V=3, T=1) == -1
    assert emit(R=1, nbytes=1 << 40) == -2 and emit(R=513, nbytes=1 << 40) == -2

    assert size(u32(0)) == 0 and size(u32(1)) == 0 and size(u32(513)) == 0
    sizes = [size(u32(R)) for R in range(2, 513)]
    assert all(b > a for a, b in zip(sizes[:-1], sizes[1:]))
    assert sizes[0] >= 10 * 8 and sizes[-1] >= 10 * 512 ** 3  # two offsets and two bytes per lattice point
    assert sizes[-1] < 2 ** 31
