"""include/pvd_hip_mesh_simplify.h -- vertex clustering -- next to the other mesh headers: the new header declares exactly three
names, libpvd_hip.so exports them, the binding lists them in a tuple of its own, and the other headers, their lists and the ABI number
are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_mesh_simplify_count", "pvd_mesh_simplify_emit", "pvd_mesh_simplify_workspace_bytes"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST", "pvd_hip.h": "ENTRY_POINTS"}


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _bytes(V, T, G, K):
    """The formula of the header's comment."""
    C = G ** 3
    return 8 * (4 + K) * min(V, C) + 4 * V + 4 * C + 4 * ((C + 255) // 256) + 4 * T + 4 * ((T + 255) // 256)


def test_the_header_declares_exactly_the_three_entry_points():
    assert _declared("pvd_hip_mesh_simplify.h") == NAMES
    src = _source("pvd_hip_mesh_simplify.h")
    assert '#include "pvd_hip.h"' in src and "#define PVD_MESH_SIMPLIFY_MAX_G 512" in src and "#define PVD_MESH_SIMPLIFY_MAX_K 8" in src
    assert "e_a / G  +  2^-30 e_a  +  2^-23 max(|bmin_a|, |bmax_a|)" in src  # the displacement bound is derived there
    assert "DUPLICATES ARE NOT MERGED" in src and "NOT GUARANTEED MANIFOLD" in src and "PROJECTED ONTO THE BOX" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh.h") == ["pvd_mesh_count", "pvd_mesh_emit", "pvd_mesh_workspace_bytes"]
    assert _declared("pvd_hip_mesh_dist.h") == ["pvd_mesh_dist_build", "pvd_mesh_dist_query", "pvd_mesh_dist_workspace_bytes"]
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_SIMPLIFY, tuple)
    assert sorted(pvd_hip.ENTRY_POINTS_MESH_SIMPLIFY) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(header), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_SIMPLIFY) & set(getattr(pvd_hip, tup)), header
    assert callable(pvd_hip.mesh_simplify_workspace_bytes) and callable(pvd_hip.mesh_simplify_count)
    assert callable(pvd_hip.mesh_simplify_emit)
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_SIMPLIFY_MAX_G == 512 and pvd_hip.MESH_SIMPLIFY_MAX_K == 8


def test_the_source_is_in_the_makefile():
    mk = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_simplify.hip" in srcs.split() and "../../include/pvd_hip_mesh_simplify.h" in mk


def test_the_workspace_size(hip_lib_built):
    import pytest
    import pvd_hip
    assert pvd_hip.mesh_simplify_workspace_bytes(0, 0, 1, 0) == 4 + 4
    assert pvd_hip.mesh_simplify_workspace_bytes(10, 7, 2, 3) == 8 * 7 * 8 + 40 + 32 + 4 + 28 + 4
    for V, T, G, K in ((0, 0, 1, 0), (10, 7, 2, 3), (1000, 3000, 41, 6), (330000, 659000, 512, 8), (2 ** 31 - 1, 2 ** 31 - 1, 512, 8)):
        assert pvd_hip.mesh_simplify_workspace_bytes(V, T, G, K) == _bytes(V, T, G, K), (V, T, G, K)
    for V, T, G, K in ((10, 10, 0, 0), (10, 10, 513, 0), (10, 10, 4, 9), (2 ** 31, 10, 4, 0), (10, 2 ** 31, 4, 0), (-1, 10, 4, 0),
                       (10, 10, 2 ** 32, 0), (10, 10, 4, -1)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_simplify_workspace_bytes(V, T, G, K)


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    n = pvd_hip.mesh_simplify_workspace_bytes(3, 1, 2, 0)
    ws = torch.zeros(n + 16, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 16:][:n]
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_simplify_count(v, t, torch.zeros(3), torch.ones(3), 2, 0, ws, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_simplify_emit(v, t, None, torch.zeros(3), torch.ones(3), 2, ws, torch.zeros(0, 3), None,
                                   torch.zeros(0, 3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    from pvd.mesh import simplify_mesh
    with pytest.raises(pvd_hip.PvdHipError):
        simplify_mesh(v, t, 2)
    with pytest.raises(pvd_hip.PvdHipError):
        simplify_mesh(v, t, 0)  # the grid is checked before any tensor
    with pytest.raises(pvd_hip.PvdHipError):
        simplify_mesh(v, t, 513)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, a short or unaligned workspace, V' above min(V, G^3) or T' above T: PVD_ERR_INVALID; G of 0 or 513, K of 9, V or T
    of 2^31: PVD_ERR_UNSUPPORTED -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, vp, sz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
    one = vp(64)  # a non-NULL, 16-byte aligned value that is never dereferenced on these paths
    size = lib.pvd_mesh_simplify_workspace_bytes
    size.restype = ctypes.c_size_t
    lib.pvd_mesh_simplify_count.restype = lib.pvd_mesh_simplify_emit.restype = ctypes.c_int

    def nbytes_of(V, T, G, K):
        return size(u32(V), u32(T), u32(G), u32(K))
    assert nbytes_of(9, 5, 0, 0) == 0 and nbytes_of(9, 5, 513, 0) == 0 and nbytes_of(9, 5, 4, 9) == 0
    assert nbytes_of(2 ** 31, 5, 4, 0) == 0 and nbytes_of(9, 2 ** 31, 4, 0) == 0 and nbytes_of(9, 5, 4, 8) == _bytes(9, 5, 4, 8)
    full = nbytes_of(9, 5, 4, 3)

    def count(verts=one, V=9, tris=one, T=5, bmin=one, bmax=one, G=4, K=3, ws=one, nbytes=None, totals=one):
        return lib.pvd_mesh_simplify_count(verts, u32(V), tris, u32(T), bmin, bmax, u32(G), u32(K), ws,
                                           sz(nbytes_of(V, T, G, K) if nbytes is None else nbytes), totals, vp(0))
    assert count(verts=vp(0)) == -1 and count(tris=vp(0)) == -1 and count(bmin=vp(0)) == -1 and count(bmax=vp(0)) == -1
    assert count(totals=vp(0)) == -1
    assert count(ws=vp(0)) == -1 and count(ws=vp(72)) == -1 and count(ws=vp(68)) == -1  # NULL, 8- and 4-byte aligned only
    assert count(nbytes=full - 1) == -1 and count(nbytes=0) == -1
    big = 1 << 40
    assert count(G=0, nbytes=big) == -2 and count(G=513, nbytes=big) == -2 and count(K=9, nbytes=big) == -2
    assert count(V=2 ** 31, nbytes=big) == -2 and count(T=2 ** 31, nbytes=big) == -2

    def emit(verts=one, V=9, tris=one, T=5, attrs=one, K=3, bmin=one, bmax=one, G=4, ws=one, nbytes=None, out_v=one, Vn=2, out_a=one,
             out_t=one, Tn=1, vmap=one):
        return lib.pvd_mesh_simplify_emit(verts, u32(V), tris, u32(T), attrs, u32(K), bmin, bmax, u32(G), ws,
                                          sz(nbytes_of(V, T, G, K) if nbytes is None else nbytes), out_v, u32(Vn), out_a, out_t, u32(Tn),
                                          vmap, vp(0))
    assert emit(verts=vp(0)) == -1 and emit(tris=vp(0)) == -1 and emit(attrs=vp(0)) == -1 and emit(bmin=vp(0)) == -1
    assert emit(bmax=vp(0)) == -1 and emit(out_v=vp(0)) == -1 and emit(out_a=vp(0)) == -1 and emit(out_t=vp(0)) == -1
    assert emit(vmap=vp(0)) == -1
    assert emit(ws=vp(0)) == -1 and emit(ws=vp(72)) == -1 and emit(nbytes=full - 1) == -1
    assert emit(Vn=10) == -1 and emit(Tn=6) == -1 and emit(G=2, Vn=9) == -1  # V' above V, T' above T, V' above G^3
    assert emit(G=0, nbytes=big) == -2 and emit(G=513, nbytes=big) == -2 and emit(K=9, nbytes=big) == -2
    assert emit(V=2 ** 31, nbytes=big) == -2 and emit(T=2 ** 31, nbytes=big) == -2
    # nothing to do: V == 0 (then T' and V' are 0) returns PVD_OK without a launch, NULL arrays allowed
    assert emit(V=0, T=0, verts=vp(0), tris=vp(0), attrs=vp(0), out_v=vp(0), out_a=vp(0), out_t=vp(0), vmap=vp(0), Vn=0, Tn=0) == 0
