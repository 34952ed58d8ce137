"""include/pvd_hip_mesh_topo.h -- topology report and clean-up -- next to the other mesh headers: the new header declares exactly four
names, libpvd_hip.so exports them, the binding lists them in a tuple of its own, and the other headers, their lists and the ABI
number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_mesh_topo_build", "pvd_mesh_topo_clean_count", "pvd_mesh_topo_clean_emit", "pvd_mesh_topo_workspace_bytes"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip_mesh_ray.h": "ENTRY_POINTS_MESH_RAY",
          "pvd_hip_mesh_smooth.h": "ENTRY_POINTS_MESH_SMOOTH", "pvd_hip_prefix.h": "ENTRY_POINTS_PREFIX", "pvd_hip.h": "ENTRY_POINTS"}


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _bytes(V, T):
    """The formula of the header's comment."""
    return 48 * V + 45 * T + 16 * ((V + 255) // 256) + 4 * ((T + 255) // 256) + 212


def test_the_header_declares_exactly_the_four_entry_points():
    assert _declared("pvd_hip_mesh_topo.h") == NAMES
    src = _source("pvd_hip_mesh_topo.h")
    assert '#include "pvd_hip.h"' in src and "#define PVD_MESH_TOPO_TOTALS 16" in src
    assert "48 V + 45 T + 16 ceil(V / 256) + 4 ceil(T / 256) + 212" in src  # the workspace formula
    for word in ("SURVIVOR", "DUPLICATE", "CANCELLED", "BOUNDARY", "INCONSISTENT", "NON-MANIFOLD", "UNBALANCED", "LABEL", "KEPT"):
        assert word in src, word
    for word in ("No re-orientation", "no hole filling", "no splitting of non-manifold vertices", "no\n *          merging of vertices by position"):
        assert word in src, word


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh_smooth.h") == ["pvd_mesh_smooth_build", "pvd_mesh_smooth_run", "pvd_mesh_smooth_workspace_bytes"]
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_TOPO, tuple)
    assert sorted(pvd_hip.ENTRY_POINTS_MESH_TOPO) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(header), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_TOPO) & set(getattr(pvd_hip, tup)), header
    for name in NAMES:
        assert callable(getattr(pvd_hip, name[4:])), name
    assert pvd_hip.ABI_VERSION == 6 and len(pvd_hip.MESH_TOPO_TOTALS) == 14
    import mesh_topo_restatement as tr
    assert pvd_hip.MESH_TOPO_TOTALS == tr.NAMES


def test_the_source_and_the_header_are_in_the_makefile():
    mk = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_topo.hip" in srcs.split() and "../../include/pvd_hip_mesh_topo.h" in mk
    src = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "mesh_topo.hip")).read()
    assert '#include "block_scan.h"' in src and "k_scan<" in src and "__shfl_up" not in src  # the shared scan, not a sixth copy


def test_the_workspace_size(hip_lib_built):
    import pytest
    import pvd_hip
    assert pvd_hip.mesh_topo_workspace_bytes(0, 0) == 212
    assert pvd_hip.mesh_topo_workspace_bytes(10, 7) == 480 + 315 + 16 + 4 + 212
    for V, T in ((0, 0), (10, 7), (255, 1), (256, 0), (257, 3000), (1, 256), (3, 257), (330000, 659000), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert pvd_hip.mesh_topo_workspace_bytes(V, T) == _bytes(V, T), (V, T)
    for V, T in ((2 ** 31, 10), (10, 2 ** 31), (-1, 10), (10, -1), (2 ** 32, 10)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_topo_workspace_bytes(V, T)


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    n = pvd_hip.mesh_topo_workspace_bytes(3, 1)
    ws = torch.zeros(n + 16, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 16:][:n]
    i64, i32 = torch.int64, torch.int32
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_topo_build(v, t, ws, torch.zeros(16, dtype=i64))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_topo_clean_count(3, 1, ws, 0, False, torch.zeros(2, dtype=i64))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_topo_clean_emit(v, t, ws, torch.zeros(3, 3), torch.zeros(1, 3, dtype=i32), torch.zeros(3, dtype=i32), torch.zeros(1, dtype=i32))
    from pvd.mesh import clean_mesh, mesh_topology
    with pytest.raises(pvd_hip.PvdHipError):
        mesh_topology(v, t)
    with pytest.raises(pvd_hip.PvdHipError):
        clean_mesh(v, t)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, a short or unaligned workspace: PVD_ERR_INVALID; V or T of 2^31: PVD_ERR_UNSUPPORTED -- all before a device is
    touched (the pointers are never dereferenced).  The optional outputs may be NULL: with everything else wrong the answer is the
    same."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, vp, sz = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
    one = vp(64)  # a non-NULL, 16-byte aligned value that is never dereferenced on these paths
    size = lib.pvd_mesh_topo_workspace_bytes
    size.restype = ctypes.c_size_t
    lib.pvd_mesh_topo_build.restype = lib.pvd_mesh_topo_clean_count.restype = lib.pvd_mesh_topo_clean_emit.restype = ctypes.c_int

    def nbytes_of(V, T):
        return size(u32(V), u32(T))
    assert nbytes_of(2 ** 31, 5) == 0 and nbytes_of(9, 2 ** 31) == 0 and nbytes_of(9, 5) == _bytes(9, 5)
    full = nbytes_of(9, 5)
    big = 1 << 40

    def build(verts=one, V=9, tris=one, T=5, ws=one, nbytes=None, totals=one, flags=one, shell=one):
        return lib.pvd_mesh_topo_build(verts, u32(V), tris, u32(T), ws, sz(nbytes_of(V, T) if nbytes is None else nbytes), totals, flags,
                                       shell, vp(0))
    for opt in (dict(), dict(flags=vp(0), shell=vp(0))):
        assert build(verts=vp(0), **opt) == -1 and build(tris=vp(0), **opt) == -1 and build(totals=vp(0), **opt) == -1
        assert build(ws=vp(0), **opt) == -1 and build(ws=vp(72), **opt) == -1 and build(ws=vp(68), **opt) == -1  # NULL, 8- and 4-byte aligned
        assert build(nbytes=full - 1, **opt) == -1 and build(nbytes=0, **opt) == -1
        assert build(V=2 ** 31, nbytes=big, **opt) == -2 and build(T=2 ** 31, nbytes=big, **opt) == -2
    assert build(V=0, totals=vp(0)) == -1 and build(T=0, totals=vp(0)) == -1  # the totals are written even for an empty mesh

    def count(V=9, T=5, ws=one, nbytes=None, least=0, largest=0, counts=one):
        return lib.pvd_mesh_topo_clean_count(u32(V), u32(T), ws, sz(nbytes_of(V, T) if nbytes is None else nbytes), u32(least), u32(largest),
                                             counts, vp(0))
    assert count(counts=vp(0)) == -1 and count(ws=vp(0)) == -1 and count(ws=vp(72)) == -1 and count(nbytes=full - 1) == -1
    assert count(V=2 ** 31, nbytes=big) == -2 and count(T=2 ** 31, nbytes=big) == -2
    assert count(V=0, counts=vp(0)) == -1

    def emit(verts=one, V=9, tris=one, T=5, ws=one, nbytes=None, out_v=one, out_t=one, vmap=one, tmap=one):
        return lib.pvd_mesh_topo_clean_emit(verts, u32(V), tris, u32(T), ws, sz(nbytes_of(V, T) if nbytes is None else nbytes), out_v, out_t,
                                            vmap, tmap, vp(0))
    assert emit(verts=vp(0)) == -1 and emit(tris=vp(0)) == -1 and emit(vmap=vp(0)) == -1 and emit(tmap=vp(0)) == -1
    assert emit(ws=vp(0)) == -1 and emit(ws=vp(72)) == -1 and emit(nbytes=full - 1) == -1
    assert emit(V=2 ** 31, nbytes=big) == -2 and emit(T=2 ** 31, nbytes=big) == -2
    assert emit(V=0, T=5, tmap=vp(0)) == -1 and emit(V=9, T=0, vmap=vp(0)) == -1
    # nothing to do at all: PVD_OK without a launch
    assert emit(V=0, T=0, verts=vp(0), tris=vp(0), ws=vp(0), nbytes=0, out_v=vp(0), out_t=vp(0), vmap=vp(0), tmap=vp(0)) == 0
