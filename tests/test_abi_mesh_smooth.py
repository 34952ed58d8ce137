"""include/pvd_hip_mesh_smooth.h -- Taubin smoothing -- next to the other mesh headers: the new header declares exactly three names,
libpvd_hip.so exports them, the binding lists them in a tuple of its own, and the other headers, their lists and the ABI number are
what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_mesh_smooth_build", "pvd_mesh_smooth_run", "pvd_mesh_smooth_workspace_bytes"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip_mesh_ray.h": "ENTRY_POINTS_MESH_RAY", "pvd_hip.h": "ENTRY_POINTS"}


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _bytes(V, T):
    """The formula of the header's comment."""
    return 64 * V + 12 * ((V + 255) // 256) + 24 * T + 24


def test_the_header_declares_exactly_the_three_entry_points():
    assert _declared("pvd_hip_mesh_smooth.h") == NAMES
    src = _source("pvd_hip_mesh_smooth.h")
    assert '#include "pvd_hip.h"' in src and "#define PVD_MESH_SMOOTH_MAX_ITERATIONS 1024" in src
    assert "64 V + 12 ceil(V / 256) + 24 T + 24" in src  # the workspace formula
    assert "2^-30 e_a  +  2^-23 max(|bmin_a|, |bmax_a|)" in src  # the round-trip bound is derived there
    assert "A NEIGHBOUR ACROSS AN EDGE SHARED BY k VALID TRIANGLES APPEARS" in src and "PROJECTED ONTO THE BOX" in src
    assert "uniform umbrella" in src and "boundary edge" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh_simplify.h") == ["pvd_mesh_simplify_count", "pvd_mesh_simplify_emit", "pvd_mesh_simplify_workspace_bytes"]
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_SMOOTH, tuple)
    assert sorted(pvd_hip.ENTRY_POINTS_MESH_SMOOTH) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(header), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_SMOOTH) & set(getattr(pvd_hip, tup)), header
    assert callable(pvd_hip.mesh_smooth_workspace_bytes) and callable(pvd_hip.mesh_smooth_build) and callable(pvd_hip.mesh_smooth_run)
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_SMOOTH_MAX_ITERATIONS == 1024


def test_the_source_is_in_the_makefile():
    mk = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_smooth.hip" in srcs.split() and "../../include/pvd_hip_mesh_smooth.h" in mk


def test_the_workspace_size(hip_lib_built):
    import pytest
    import pvd_hip
    assert pvd_hip.mesh_smooth_workspace_bytes(0, 0) == 24
    assert pvd_hip.mesh_smooth_workspace_bytes(10, 7) == 640 + 12 + 168 + 24
    for V, T in ((0, 0), (10, 7), (255, 1), (256, 0), (257, 3000), (330000, 659000), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert pvd_hip.mesh_smooth_workspace_bytes(V, T) == _bytes(V, T), (V, T)
    for V, T in ((2 ** 31, 10), (10, 2 ** 31), (-1, 10), (10, -1), (2 ** 32, 10)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_smooth_workspace_bytes(V, T)


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    n = pvd_hip.mesh_smooth_workspace_bytes(3, 1)
    ws = torch.zeros(n + 16, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 16:][:n]
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_smooth_build(v, t, torch.zeros(3), torch.ones(3), None, ws, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_smooth_run(v, 1, torch.zeros(3), torch.ones(3), ws, 0.5, -0.53, 1, torch.zeros(3, 3))
    from pvd.mesh import smooth_mesh
    with pytest.raises(pvd_hip.PvdHipError):
        smooth_mesh(v, t, 2)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """NULL pointers, a short or unaligned workspace, a weight that is not finite or above 1, iterations above the limit:
    PVD_ERR_INVALID; V or T of 2^31: PVD_ERR_UNSUPPORTED -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, vp, sz, dbl = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    one = vp(64)  # a non-NULL, 16-byte aligned value that is never dereferenced on these paths
    size = lib.pvd_mesh_smooth_workspace_bytes
    size.restype = ctypes.c_size_t
    lib.pvd_mesh_smooth_build.restype = lib.pvd_mesh_smooth_run.restype = ctypes.c_int

    def nbytes_of(V, T):
        return size(u32(V), u32(T))
    assert nbytes_of(2 ** 31, 5) == 0 and nbytes_of(9, 2 ** 31) == 0 and nbytes_of(9, 5) == _bytes(9, 5)
    full = nbytes_of(9, 5)
    big = 1 << 40

    def build(verts=one, V=9, tris=one, T=5, bmin=one, bmax=one, pinned=one, ws=one, nbytes=None, totals=one):
        return lib.pvd_mesh_smooth_build(verts, u32(V), tris, u32(T), bmin, bmax, pinned, ws, sz(nbytes_of(V, T) if nbytes is None else nbytes),
                                         totals, vp(0))
    assert build(verts=vp(0)) == -1 and build(tris=vp(0)) == -1 and build(bmin=vp(0)) == -1 and build(bmax=vp(0)) == -1
    assert build(totals=vp(0)) == -1
    assert build(ws=vp(0)) == -1 and build(ws=vp(72)) == -1 and build(ws=vp(68)) == -1  # NULL, 8- and 4-byte aligned only
    assert build(nbytes=full - 1) == -1 and build(nbytes=0) == -1
    assert build(V=2 ** 31, nbytes=big) == -2 and build(T=2 ** 31, nbytes=big) == -2
    # nothing to do: V == 0 returns PVD_OK without a launch, NULL arrays allowed
    assert build(V=0, T=0, verts=vp(0), tris=vp(0), pinned=vp(0), ws=vp(0), totals=vp(0), bmin=vp(0), bmax=vp(0), nbytes=0) == 0
    assert build(V=0, T=5, verts=vp(0), pinned=vp(0)) == 0

    def run(verts=one, V=9, T=5, bmin=one, bmax=one, ws=one, nbytes=None, lam=0.5, mu=-0.53, iterations=3, out=one):
        return lib.pvd_mesh_smooth_run(verts, u32(V), u32(T), bmin, bmax, ws, sz(nbytes_of(V, T) if nbytes is None else nbytes), dbl(lam),
                                       dbl(mu), u32(iterations), out, vp(0))
    assert run(verts=vp(0)) == -1 and run(bmin=vp(0)) == -1 and run(bmax=vp(0)) == -1 and run(out=vp(0)) == -1
    assert run(ws=vp(0)) == -1 and run(ws=vp(72)) == -1 and run(nbytes=full - 1) == -1
    nan, inf = float("nan"), float("inf")
    assert run(lam=nan) == -1 and run(mu=nan) == -1 and run(lam=inf) == -1 and run(mu=-inf) == -1
    assert run(lam=1.0000001) == -1 and run(mu=-1.0000001) == -1
    assert run(iterations=1025) == -1 and run(iterations=2 ** 32 - 1) == -1
    assert run(V=2 ** 31, nbytes=big) == -2 and run(T=2 ** 31, nbytes=big) == -2
    assert run(V=0, T=0, verts=vp(0), ws=vp(0), out=vp(0), bmin=vp(0), bmax=vp(0), nbytes=0) == 0
