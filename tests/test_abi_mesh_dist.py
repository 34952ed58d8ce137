"""include/pvd_hip_mesh_dist.h -- the point-to-mesh distance -- next to the other mesh headers: the new header declares exactly three
names, libpvd_hip.so exports them, the binding lists them in a tuple of its own, and the other headers, their lists and the ABI number
are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_mesh_dist_build", "pvd_mesh_dist_query", "pvd_mesh_dist_workspace_bytes"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip.h": "ENTRY_POINTS"}


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_header_declares_exactly_the_three_entry_points():
    assert _declared("pvd_hip_mesh_dist.h") == NAMES
    src = _source("pvd_hip_mesh_dist.h")
    assert '#include "pvd_hip.h"' in src and "#define PVD_MESH_DIST_MAX_G 256" in src
    assert "r h_min - rho" in src  # the bound of the ring search is derived there


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh.h") == ["pvd_mesh_count", "pvd_mesh_emit", "pvd_mesh_workspace_bytes"]
    assert _declared("pvd_hip_mesh_attr.h") == ["pvd_mesh_normals"]
    assert _declared("pvd_hip_components.h") == ["pvd_components_filter", "pvd_components_label", "pvd_components_neighbours"]
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_DIST, tuple)
    assert sorted(pvd_hip.ENTRY_POINTS_MESH_DIST) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(header), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_DIST) & set(getattr(pvd_hip, tup)), header
    assert callable(pvd_hip.mesh_dist_workspace_bytes) and callable(pvd_hip.mesh_dist_build) and callable(pvd_hip.mesh_dist_query)
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_DIST_MAX_G == 256


def test_the_source_is_in_the_makefile():
    mk = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_dist.hip" in srcs.split() and "../../include/pvd_hip_mesh_dist.h" in mk


def test_the_workspace_size(hip_lib_built):
    import pytest
    import pvd_hip
    # header 64, 48 + 4 per triangle, (G^3 + 1) starts, G^3 cursors, one sum per 256 cells
    assert pvd_hip.mesh_dist_workspace_bytes(0, 1) == 64 + 8 + 4 + 4
    assert pvd_hip.mesh_dist_workspace_bytes(10, 2) == 64 + 520 + 36 + 32 + 4
    assert pvd_hip.mesh_dist_workspace_bytes(1000, 256) == 64 + 52000 + 4 * (2 * 256 ** 3 + 1) + 4 * 65536
    for T, G in ((10, 0), (10, 257), (2 ** 31, 4), (-1, 4), (10, 2 ** 32)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_dist_workspace_bytes(T, G)


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    ws = torch.zeros(pvd_hip.mesh_dist_workspace_bytes(1, 2) + 16, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 16:][:pvd_hip.mesh_dist_workspace_bytes(1, 2)]
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_dist_build(v, t, torch.zeros(3), torch.ones(3), 2, ws)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_dist_query(torch.zeros(4, 3), 1, 2, ws, 1.0, torch.zeros(4), torch.zeros(4, dtype=torch.int32))
    from pvd.mesh import mesh_distance
    with pytest.raises(pvd_hip.PvdHipError):
        mesh_distance(torch.zeros(4, 3), v, t, 1.0)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, a short or unaligned workspace: PVD_ERR_INVALID; G of 0 or 257 (and T of 2^31): PVD_ERR_UNSUPPORTED; max_dist
    <= 0, infinite or NaN: PVD_ERR_INVALID; N == 0: PVD_OK -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp, sz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    one = vp(64)  # a non-NULL, 16-byte aligned value that is never dereferenced on these paths
    size = lib.pvd_mesh_dist_workspace_bytes
    size.restype = ctypes.c_size_t
    lib.pvd_mesh_dist_build.restype = lib.pvd_mesh_dist_query.restype = ctypes.c_int
    assert size(u32(5), u32(0)) == 0 and size(u32(5), u32(257)) == 0 and size(u32(2 ** 31), u32(4)) == 0 and size(u32(5), u32(4)) > 0

    def query(points=one, N=0, T=5, G=4, ws=one, nbytes=None, max_dist=1.0, dist=one, tri=one):
        return lib.pvd_mesh_dist_query(points, u32(N), u32(T), u32(G), ws, sz(size(u32(T), u32(G)) if nbytes is None else nbytes),
                                       f32(max_dist), dist, tri, vp(0))
    assert query() == 0 and query(points=vp(0), dist=vp(0), tri=vp(0)) == 0  # N == 0: nothing to do
    assert query(T=0) == 0
    assert query(ws=vp(0)) == -1 and query(ws=vp(72)) == -1 and query(ws=vp(68)) == -1  # NULL, 8- and 4-byte aligned only
    assert query(nbytes=size(u32(5), u32(4)) - 1) == -1 and query(nbytes=0) == -1
    assert query(G=0, nbytes=1 << 40) == -2 and query(G=257, nbytes=1 << 40) == -2 and query(T=2 ** 31, nbytes=1 << 40) == -2
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert query(max_dist=bad) == -1 and query(max_dist=bad, N=7) == -1
    assert query(N=7, points=vp(0)) == -1 and query(N=7, dist=vp(0)) == -1 and query(N=7, tri=vp(0)) == -1
    assert query(N=7, G=257, nbytes=1 << 40) == -2 and query(N=7, ws=vp(0)) == -1  # with points too: the checks come first

    def build(verts=one, V=9, tris=one, T=5, bmin=one, bmax=one, G=4, ws=one, nbytes=None):
        return lib.pvd_mesh_dist_build(verts, u32(V), tris, u32(T), bmin, bmax, u32(G), ws,
                                       sz(size(u32(T), u32(G)) if nbytes is None else nbytes), vp(0))
    assert build(verts=vp(0)) == -1 and build(tris=vp(0)) == -1 and build(bmin=vp(0)) == -1 and build(bmax=vp(0)) == -1
    assert build(ws=vp(0)) == -1 and build(ws=vp(72)) == -1 and build(nbytes=size(u32(5), u32(4)) - 1) == -1
    assert build(G=0, nbytes=1 << 40) == -2 and build(G=257, nbytes=1 << 40) == -2 and build(T=2 ** 31, nbytes=1 << 40) == -2
