"""include/pvd_hip_mesh_ray.h -- ray casting against a mesh -- next to the other mesh headers: the new header declares exactly four
names, libpvd_hip.so exports them, the binding lists them in a tuple of its own, and the other headers, their lists and the ABI number
are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_mesh_ray_build", "pvd_mesh_ray_cast", "pvd_mesh_ray_count", "pvd_mesh_ray_workspace_bytes"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip.h": "ENTRY_POINTS"}


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _bytes(T, G, pairs):
    """The formula of the header's comment."""
    C = G ** 3
    return 64 + 48 * T + 4 * (C + 1) + 4 * C + 4 * ((C + 255) // 256) + 4 * T + 4 * pairs


def test_the_header_declares_exactly_the_four_entry_points():
    assert _declared("pvd_hip_mesh_ray.h") == NAMES
    src = _source("pvd_hip_mesh_ray.h")
    assert '#include "pvd_hip.h"' in src and "#define PVD_MESH_RAY_MAX_G 256" in src
    assert "NO PRODUCT IS FUSED INTO A SUM" in src and "t = ((U * Za + V * Zb) + W * Zc) / det" in src
    assert "WHY NO WINNER IS MISSED" in src  # the walk's argument is derived there


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh_dist.h") == ["pvd_mesh_dist_build", "pvd_mesh_dist_query", "pvd_mesh_dist_workspace_bytes"]
    assert _declared("pvd_hip_mesh_simplify.h") == ["pvd_mesh_simplify_count", "pvd_mesh_simplify_emit", "pvd_mesh_simplify_workspace_bytes"]
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_RAY, tuple) and len(pvd_hip.ENTRY_POINTS_MESH_RAY) == 4
    assert sorted(pvd_hip.ENTRY_POINTS_MESH_RAY) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(header), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_RAY) & set(getattr(pvd_hip, tup)), header
    assert callable(pvd_hip.mesh_ray_workspace_bytes) and callable(pvd_hip.mesh_ray_count)
    assert callable(pvd_hip.mesh_ray_build) and callable(pvd_hip.mesh_ray_cast)
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_RAY_MAX_G == 256


def test_the_source_is_in_the_makefile():
    mk = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_ray.hip" in srcs.split() and "../../include/pvd_hip_mesh_ray.h" in mk and " mesh_tri_grid.h " in mk
    # the grid is built by the header it shares with the winding numbers, not by a copy
    assert "int classify(" not in open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "mesh_ray.hip")).read()


def test_the_workspace_size(hip_lib_built):
    import pytest
    import pvd_hip
    assert pvd_hip.mesh_ray_workspace_bytes(0, 1, 0) == 64 + 8 + 4 + 4
    for T, G, pairs in ((0, 1, 0), (7, 2, 19), (11000, 37, 52000), (2 ** 31 - 1, 256, 2 ** 31 - 1)):
        assert pvd_hip.mesh_ray_workspace_bytes(T, G, pairs) == _bytes(T, G, pairs), (T, G, pairs)
    for T, G, pairs in ((10, 0, 5), (10, 257, 5), (2 ** 31, 4, 5), (10, 4, 2 ** 31), (-1, 4, 5), (10, 2 ** 32, 5), (10, 4, -1), (10, 4, 2 ** 64)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_ray_workspace_bytes(T, G, pairs)


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    lo, hi = torch.zeros(3), torch.ones(3)
    n = pvd_hip.mesh_ray_workspace_bytes(1, 2, 8)
    ws = torch.zeros(n + 16, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 16:][:n]
    o, d = torch.zeros(5, 3), torch.ones(5, 3)
    out = (torch.zeros(5), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 2))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_ray_count(v, t, lo, hi, 2, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_ray_build(v, t, lo, hi, 2, 8, ws)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_ray_cast(o, d, 1, 2, 8, ws, 0.0, 1.0, *out)
    from pvd.mesh import mesh_raycast
    with pytest.raises(pvd_hip.PvdHipError):
        mesh_raycast(o, d, v, t)

    # arguments checked before any tensor is looked at
    for T, G, pairs in ((1, 0, 8), (1, 257, 8), (1, 2, 2 ** 31)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_ray_workspace_bytes(T, G, pairs)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_ray_cast(o, d.reshape(-1), 1, 2, 8, ws, 0.0, 1.0, *out)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, a short or unaligned workspace, a bad t_min or t_max: PVD_ERR_INVALID; G of 0 or 257, T or pairs of 2^31:
    PVD_ERR_UNSUPPORTED; N == 0: PVD_OK -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, u64, vp, sz, f32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
    one = vp(64)  # a non-NULL, 16-byte aligned value that is never dereferenced on these paths
    size = lib.pvd_mesh_ray_workspace_bytes
    size.restype = ctypes.c_size_t
    lib.pvd_mesh_ray_count.restype = lib.pvd_mesh_ray_build.restype = lib.pvd_mesh_ray_cast.restype = ctypes.c_int

    def nbytes_of(T, G, pairs):
        return size(u32(T), u32(G), u64(pairs))
    assert nbytes_of(5, 0, 9) == 0 and nbytes_of(5, 257, 9) == 0 and nbytes_of(2 ** 31, 4, 9) == 0 and nbytes_of(5, 4, 2 ** 31) == 0
    assert nbytes_of(5, 4, 9) == _bytes(5, 4, 9) and nbytes_of(5, 256, 2 ** 31 - 1) == _bytes(5, 256, 2 ** 31 - 1)
    full = nbytes_of(5, 4, 9)
    big = 1 << 40
    inf, nan = float("inf"), float("nan")

    def count(verts=one, V=9, tris=one, T=5, bmin=one, bmax=one, G=4, totals=one):
        return lib.pvd_mesh_ray_count(verts, u32(V), tris, u32(T), bmin, bmax, u32(G), totals, vp(0))
    assert count(verts=vp(0)) == -1 and count(tris=vp(0)) == -1 and count(bmin=vp(0)) == -1 and count(bmax=vp(0)) == -1
    assert count(totals=vp(0)) == -1
    assert count(G=0) == -2 and count(G=257) == -2 and count(T=2 ** 31) == -2

    def build(verts=one, V=9, tris=one, T=5, bmin=one, bmax=one, G=4, pairs=9, ws=one, nbytes=None):
        return lib.pvd_mesh_ray_build(verts, u32(V), tris, u32(T), bmin, bmax, u32(G), u64(pairs), ws,
                                      sz(nbytes_of(T, G, pairs) if nbytes is None else nbytes), vp(0))
    assert build(verts=vp(0)) == -1 and build(tris=vp(0)) == -1 and build(bmin=vp(0)) == -1 and build(bmax=vp(0)) == -1
    assert build(ws=vp(0)) == -1 and build(ws=vp(72)) == -1 and build(ws=vp(68)) == -1  # NULL, 8- and 4-byte aligned only
    assert build(nbytes=full - 1) == -1 and build(nbytes=0) == -1
    assert build(G=0, nbytes=big) == -2 and build(G=257, nbytes=big) == -2 and build(T=2 ** 31, nbytes=big) == -2
    assert build(pairs=2 ** 31, nbytes=big) == -2

    def cast(o=one, d=one, N=7, T=5, G=4, pairs=9, ws=one, nbytes=None, t_min=0.0, t_max=inf, t=one, tri=one, bary=one):
        return lib.pvd_mesh_ray_cast(o, d, u32(N), u32(T), u32(G), u64(pairs), ws, sz(nbytes_of(T, G, pairs) if nbytes is None else nbytes),
                                     f32(t_min), f32(t_max), t, tri, bary, vp(0))
    assert cast(o=vp(0)) == -1 and cast(d=vp(0)) == -1 and cast(t=vp(0)) == -1 and cast(tri=vp(0)) == -1 and cast(bary=vp(0)) == -1
    assert cast(t_min=-1.0) == -1 and cast(t_min=-1e-30) == -1 and cast(t_min=inf) == -1 and cast(t_min=nan) == -1
    assert cast(t_min=1.0, t_max=1.0) == -1 and cast(t_min=2.0, t_max=1.0) == -1 and cast(t_max=nan) == -1 and cast(t_max=0.0) == -1
    assert cast(ws=vp(0)) == -1 and cast(ws=vp(72)) == -1 and cast(nbytes=full - 1) == -1 and cast(nbytes=0) == -1
    assert cast(G=0, nbytes=big) == -2 and cast(G=257, nbytes=big) == -2 and cast(T=2 ** 31, nbytes=big) == -2
    assert cast(pairs=2 ** 31, nbytes=big) == -2
    # the interval is checked first, the workspace next, N == 0 then: PVD_OK without a launch, NULL rays and results allowed
    assert cast(N=0, o=vp(0), d=vp(0), t=vp(0), tri=vp(0), bary=vp(0)) == 0
    assert cast(N=0, t_min=0.5, t_max=inf) == 0 and cast(N=0, t_max=nan) == -1 and cast(N=0, ws=vp(0)) == -1
