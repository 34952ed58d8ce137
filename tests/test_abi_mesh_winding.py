"""include/pvd_hip_mesh_winding.h -- winding numbers -- next to the other mesh headers: the new header declares exactly five names,
libpvd_hip.so exports them, the binding lists them in a tuple of its own, and the other headers, their lists and the ABI number are
what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_mesh_winding_build", "pvd_mesh_winding_count", "pvd_mesh_winding_lattice", "pvd_mesh_winding_points",
         "pvd_mesh_winding_workspace_bytes"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip_mesh_ray.h": "ENTRY_POINTS_MESH_RAY",
          "pvd_hip_mesh_smooth.h": "ENTRY_POINTS_MESH_SMOOTH", "pvd_hip_mesh_topo.h": "ENTRY_POINTS_MESH_TOPO",
          "pvd_hip_prefix.h": "ENTRY_POINTS_PREFIX", "pvd_hip.h": "ENTRY_POINTS"}


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _bytes(T, G, pairs):
    """The formula of the header's comment."""
    C = G ** 2
    return 64 + 48 * T + 4 * (C + 1) + 4 * C + 4 * ((C + 255) // 256) + 4 * T + 4 * pairs


def test_the_header_declares_exactly_the_five_entry_points():
    assert _declared("pvd_hip_mesh_winding.h") == NAMES
    src = _source("pvd_hip_mesh_winding.h")
    assert '#include "pvd_hip.h"' in src and "#define PVD_MESH_WINDING_MAX_G 1024" in src and "#define PVD_MESH_WINDING_MAX_R 1024" in src
    assert "#define PVD_MESH_WINDING_INVALID (-2147483647 - 1)" in src
    assert "64 + 48 T + 4 (G^2 + 1) + 4 G^2 + 4 ceil(G^2 / 256) + 4 T + 4 pairs" in src  # the workspace formula
    assert "NO PRODUCT IS FUSED INTO A SUM" in src and "E(p) = (xw - xu) * (py - yu) - (yw - yu) * (px - xu)" in src
    assert "z_hit = ((e_bc * za + e_ca * zb) + e_ab * zc) / ((e_bc + e_ca) + e_ab)" in src
    assert "bitwise negations of one number" in src and "cannot slip between two triangles" in src  # why a closed mesh does not leak
    assert "e == 0 and (dy > 0, or dy == 0 and dx < 0)" in src  # the tie rule
    assert "EXACTLY ON THE SURFACE is decided by the rule above, not by geometry" in src
    assert "OPEN or INCONSISTENTLY ORIENTED" in src and "depend on the direction of the ray" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh_ray.h") == ["pvd_mesh_ray_build", "pvd_mesh_ray_cast", "pvd_mesh_ray_count", "pvd_mesh_ray_workspace_bytes"]
    assert _declared("pvd_hip_mesh_topo.h") == ["pvd_mesh_topo_build", "pvd_mesh_topo_clean_count", "pvd_mesh_topo_clean_emit",
                                                "pvd_mesh_topo_workspace_bytes"]
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_WINDING, tuple) and len(pvd_hip.ENTRY_POINTS_MESH_WINDING) == 5
    assert sorted(pvd_hip.ENTRY_POINTS_MESH_WINDING) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(header), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_WINDING) & set(getattr(pvd_hip, tup)), header
    for name in NAMES:
        assert callable(getattr(pvd_hip, name[4:])), name
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_WINDING_MAX_G == 1024 and pvd_hip.MESH_WINDING_MAX_R == 1024
    assert pvd_hip.MESH_WINDING_INVALID == -2 ** 31
    import mesh_winding_restatement as wr
    assert pvd_hip.MESH_WINDING_TOTALS == wr.TOTALS and int(wr.INVALID) == pvd_hip.MESH_WINDING_INVALID


def test_the_source_and_the_header_are_in_the_makefile():
    mk = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_winding.hip" in srcs.split() and "../../include/pvd_hip_mesh_winding.h" in mk
    assert " mesh_tri_grid.h " in mk
    src = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "mesh_winding.hip")).read()
    grid = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "mesh_tri_grid.h")).read()
    # the shared scan, not a further copy (launched by the shared build of the grid); the products are never fused by the source
    assert '#include "block_scan.h"' in grid and "k_scan<" in grid and "wave_scan(" in src and "__shfl_up" not in src
    assert "int classify(" not in src
    assert "fma(" not in src and "fmaf(" not in src and "fma(" not in grid and "fmaf(" not in grid


def test_the_workspace_size(hip_lib_built):
    import pytest
    import pvd_hip
    assert pvd_hip.mesh_winding_workspace_bytes(0, 1, 0) == 64 + 8 + 4 + 4
    for T, G, pairs in ((0, 1, 0), (7, 2, 19), (11000, 37, 52000), (5, 256, 9), (5, 257, 9), (2 ** 31 - 1, 1024, 2 ** 31 - 1)):
        assert pvd_hip.mesh_winding_workspace_bytes(T, G, pairs) == _bytes(T, G, pairs), (T, G, pairs)
    for T, G, pairs in ((10, 0, 5), (10, 1025, 5), (2 ** 31, 4, 5), (10, 4, 2 ** 31), (-1, 4, 5), (10, 2 ** 32, 5), (10, 4, -1), (10, 4, 2 ** 64)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_winding_workspace_bytes(T, G, pairs)


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    lo, hi = torch.zeros(3), torch.ones(3)
    n = pvd_hip.mesh_winding_workspace_bytes(1, 2, 8)
    ws = torch.zeros(n + 16, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 16:][:n]
    p, w = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32)
    vol, totals = torch.zeros(27, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_winding_count(v, t, lo, hi, 2, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_winding_build(v, t, lo, hi, 2, 8, ws)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_winding_points(p, 1, 2, 8, ws, w)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_winding_lattice(3, lo, hi, 1, 2, 8, ws, vol, totals)
    from pvd.mesh import compare_meshes, mesh_contains, mesh_signed_distance, mesh_to_sdf, mesh_winding, voxelize_mesh
    for call in (lambda: mesh_winding(p, v, t), lambda: mesh_contains(p, v, t), lambda: voxelize_mesh(v, t, 3, lo, hi),
                 lambda: mesh_signed_distance(p, v, t, 1.0), lambda: mesh_to_sdf(v, t, 3, lo, hi, 1.0)):
        with pytest.raises(pvd_hip.PvdHipError):
            call()
    import inspect
    assert inspect.signature(compare_meshes).parameters["volume"].default == 0  # off unless asked for


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, a short or unaligned workspace: PVD_ERR_INVALID; G of 0 or 1025, T or pairs of 2^31, R of 1 or 1025:
    PVD_ERR_UNSUPPORTED; N == 0: PVD_OK -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, u64, vp, sz = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t
    one = vp(64)  # a non-NULL, 16-byte aligned value that is never dereferenced on these paths
    size = lib.pvd_mesh_winding_workspace_bytes
    size.restype = ctypes.c_size_t
    for name in NAMES[:4]:
        getattr(lib, name).restype = ctypes.c_int

    def nbytes_of(T, G, pairs):
        return size(u32(T), u32(G), u64(pairs))
    assert nbytes_of(5, 0, 9) == 0 and nbytes_of(5, 1025, 9) == 0 and nbytes_of(2 ** 31, 4, 9) == 0 and nbytes_of(5, 4, 2 ** 31) == 0
    assert nbytes_of(5, 4, 9) == _bytes(5, 4, 9) and nbytes_of(5, 1024, 2 ** 31 - 1) == _bytes(5, 1024, 2 ** 31 - 1)
    full = nbytes_of(5, 4, 9)
    big = 1 << 40

    def count(verts=one, V=9, tris=one, T=5, bmin=one, bmax=one, G=4, totals=one):
        return lib.pvd_mesh_winding_count(verts, u32(V), tris, u32(T), bmin, bmax, u32(G), totals, vp(0))
    assert count(verts=vp(0)) == -1 and count(tris=vp(0)) == -1 and count(bmin=vp(0)) == -1 and count(bmax=vp(0)) == -1
    assert count(totals=vp(0)) == -1
    assert count(G=0) == -2 and count(G=1025) == -2 and count(T=2 ** 31) == -2

    def build(verts=one, V=9, tris=one, T=5, bmin=one, bmax=one, G=4, pairs=9, ws=one, nbytes=None):
        return lib.pvd_mesh_winding_build(verts, u32(V), tris, u32(T), bmin, bmax, u32(G), u64(pairs), ws,
                                          sz(nbytes_of(T, G, pairs) if nbytes is None else nbytes), vp(0))
    assert build(verts=vp(0)) == -1 and build(tris=vp(0)) == -1 and build(bmin=vp(0)) == -1 and build(bmax=vp(0)) == -1
    assert build(ws=vp(0)) == -1 and build(ws=vp(72)) == -1 and build(ws=vp(68)) == -1  # NULL, 8- and 4-byte aligned only
    assert build(nbytes=full - 1) == -1 and build(nbytes=0) == -1
    assert build(G=0, nbytes=big) == -2 and build(G=1025, nbytes=big) == -2 and build(T=2 ** 31, nbytes=big) == -2
    assert build(pairs=2 ** 31, nbytes=big) == -2

    def points(p=one, N=7, T=5, G=4, pairs=9, ws=one, nbytes=None, w=one):
        return lib.pvd_mesh_winding_points(p, u32(N), u32(T), u32(G), u64(pairs), ws, sz(nbytes_of(T, G, pairs) if nbytes is None else nbytes),
                                           w, vp(0))
    assert points(p=vp(0)) == -1 and points(w=vp(0)) == -1
    assert points(ws=vp(0)) == -1 and points(ws=vp(72)) == -1 and points(nbytes=full - 1) == -1 and points(nbytes=0) == -1
    assert points(G=0, nbytes=big) == -2 and points(G=1025, nbytes=big) == -2 and points(T=2 ** 31, nbytes=big) == -2
    assert points(pairs=2 ** 31, nbytes=big) == -2
    # the workspace is checked first, N == 0 then: PVD_OK without a launch, NULL points and results allowed
    assert points(N=0, p=vp(0), w=vp(0)) == 0 and points(N=0, ws=vp(0)) == -1 and points(N=0, nbytes=full - 1) == -1

    def lattice(R=9, lo=one, hi=one, T=5, G=4, pairs=9, ws=one, nbytes=None, w=one, totals=one):
        return lib.pvd_mesh_winding_lattice(u32(R), lo, hi, u32(T), u32(G), u64(pairs), ws, sz(nbytes_of(T, G, pairs) if nbytes is None else nbytes),
                                            w, totals, vp(0))
    assert lattice(lo=vp(0)) == -1 and lattice(hi=vp(0)) == -1 and lattice(w=vp(0)) == -1 and lattice(totals=vp(0)) == -1
    assert lattice(ws=vp(0)) == -1 and lattice(ws=vp(72)) == -1 and lattice(nbytes=full - 1) == -1 and lattice(nbytes=0) == -1
    assert lattice(G=0, nbytes=big) == -2 and lattice(G=1025, nbytes=big) == -2 and lattice(T=2 ** 31, nbytes=big) == -2
    assert lattice(pairs=2 ** 31, nbytes=big) == -2
    assert lattice(R=0) == -2 and lattice(R=1) == -2 and lattice(R=1025) == -2
