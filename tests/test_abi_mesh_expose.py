"""csrc/pvd_hip_mesh_expose.h -- the exposure query -- next to the other mesh headers: the new header declares exactly one name and one
constant, libpvd_hip.so exports it, the binding lists it in a tuple of its own, and the headers of include/, their lists and the ABI
number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU).  The header lives next to
its source: tests/test_abi_mesh_tex.py pins the list of files in include/."""
import ctypes
import inspect
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "aaai2023-pvd_amd", "csrc")
NAMES = ["pvd_mesh_expose"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip_mesh_ray.h": "ENTRY_POINTS_MESH_RAY",
          "pvd_hip_mesh_smooth.h": "ENTRY_POINTS_MESH_SMOOTH", "pvd_hip_mesh_topo.h": "ENTRY_POINTS_MESH_TOPO",
          "pvd_hip_mesh_winding.h": "ENTRY_POINTS_MESH_WINDING", "pvd_hip_mesh_tex.h": "ENTRY_POINTS_MESH_TEX",
          "pvd_hip_prefix.h": "ENTRY_POINTS_PREFIX", "pvd_hip.h": "ENTRY_POINTS"}


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _include(header):
    return os.path.join(REPO, "include", header)


def test_the_header_declares_exactly_the_entry_point_and_the_constant():
    path = os.path.join(CSRC, "pvd_hip_mesh_expose.h")
    assert _declared(path) == NAMES
    src = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert dict(re.findall(r"^#define (PVD_MESH_EXPOSE_[A-Z_]+) (\S+)$", code, flags=re.M)) == {"PVD_MESH_EXPOSE_MAX_D": "1024"}
    assert '#include "../../include/pvd_hip_mesh_ray.h"' in code
    # the definition is in the header: the point, the side, blocked, the proviso of the ray header
    assert "o = (float)((wa * a + wb * b) + wc * c)" in src and "NOTHING IS FUSED" in src
    assert "s = (n_x * d_x + n_y * d_y) + n_z * d_z" in src and "g != f compares INDICES" in src
    assert "THE POINT OF THE TRIANGLE" in src and "edge-on" in src


def test_the_library_exports_it_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared(_include("pvd_hip.h"))) == 75
    assert _declared(_include("pvd_hip_mesh_ray.h")) == ["pvd_mesh_ray_build", "pvd_mesh_ray_cast", "pvd_mesh_ray_count",
                                                        "pvd_mesh_ray_workspace_bytes"]
    assert set(OTHERS) == set(os.listdir(os.path.join(REPO, "include")))
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(_include(h))), h
        assert "PVD_MESH_EXPOSE_" not in open(_include(h)).read(), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_it_in_a_tuple_of_its_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_EXPOSE, tuple) and sorted(pvd_hip.ENTRY_POINTS_MESH_EXPOSE) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(_include(header)), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_EXPOSE) & set(getattr(pvd_hip, tup)), header
    assert callable(pvd_hip.mesh_expose)
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_EXPOSE_MAX_D == 1024
    import mesh_expose_restatement as er
    assert er.MAX_D == 1024 and tuple(pvd_hip.MESH_EXPOSE_TOTALS) == er.TOTALS


def test_the_source_and_the_headers_are_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_expose.hip" in srcs.split() and " pvd_hip_mesh_expose.h " in mk and " mesh_ray_walk.h " in mk
    assert "-ffp-contract=off" in [ln for ln in mk.splitlines() if ln.startswith("FLAGS")][0]
    # the walk and the test exist once, in the header both translation units include
    walk = open(os.path.join(CSRC, "mesh_ray_walk.h")).read()
    assert "const double U = Xc * Yb - Yc * Xb" in walk and "void walk(" in walk
    for name in ("mesh_ray.hip", "mesh_expose.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert '#include "mesh_ray_walk.h"' in src and "Xc * Yb" not in src and "t_exit = te" not in src, name
        assert "fma(" not in src and "fmaf(" not in src and "__shared__" not in src, name


def test_the_entry_point_checks_its_arguments_before_any_launch(hip_lib_built):
    """D outside 1 .. 1024 or S other than 1 or 4: PVD_ERR_UNSUPPORTED; then the workspace (NULL, unaligned, short: PVD_ERR_INVALID; G, T,
    pairs out of range: PVD_ERR_UNSUPPORTED); then a band outside 0 <= tri0 <= tri1 <= T: PVD_ERR_INVALID; an empty band: PVD_OK with no
    launch, NULL pointers allowed; then NULL pointers: PVD_ERR_INVALID -- all before a device is touched (the pointers are never
    dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, u64, vp, sz = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t
    one = vp(64)
    lib.pvd_mesh_expose.restype = ctypes.c_int
    lib.pvd_mesh_ray_workspace_bytes.restype = ctypes.c_size_t

    def expose(dirs=one, D=64, S=1, tri0=0, tri1=5, T=5, G=4, pairs=9, ws=one, nbytes=None, counts=one, totals=one):
        if nbytes is None:
            nbytes = lib.pvd_mesh_ray_workspace_bytes(u32(T), u32(G), u64(pairs))
        return lib.pvd_mesh_expose(dirs, u32(D), u32(S), u32(tri0), u32(tri1), u32(T), u32(G), u64(pairs), ws, sz(nbytes), counts, totals, vp(0))
    full = lib.pvd_mesh_ray_workspace_bytes(u32(5), u32(4), u64(9))
    big = 1 << 40
    assert expose(D=0) == -2 and expose(D=1025) == -2 and expose(S=0) == -2 and expose(S=2) == -2 and expose(S=3) == -2 and expose(S=5) == -2
    assert expose(D=0, ws=vp(0)) == -2  # the limits first
    assert expose(ws=vp(0)) == -1 and expose(ws=vp(72)) == -1 and expose(ws=vp(68)) == -1
    assert expose(nbytes=full - 1) == -1 and expose(nbytes=0) == -1
    assert expose(G=0, nbytes=big) == -2 and expose(G=257, nbytes=big) == -2 and expose(T=2 ** 31, nbytes=big) == -2
    assert expose(pairs=2 ** 31, nbytes=big) == -2
    assert expose(tri0=3, tri1=2) == -1 and expose(tri0=0, tri1=6) == -1 and expose(tri0=6, tri1=6) == -1
    assert expose(tri0=5, tri1=5) == 0 and expose(tri0=2, tri1=2, dirs=vp(0), counts=vp(0), totals=vp(0)) == 0
    assert expose(T=0, tri0=0, tri1=0, dirs=vp(0), counts=vp(0), totals=vp(0)) == 0
    assert expose(dirs=vp(0)) == -1 and expose(counts=vp(0)) == -1 and expose(totals=vp(0)) == -1
    assert expose(D=1, S=4, tri0=5, tri1=5) == 0 and expose(D=1024, tri0=5, tri1=5) == 0


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import torch
    import pvd_hip
    from pvd import mesh
    n = pvd_hip.mesh_ray_workspace_bytes(1, 2, 8)
    ws = torch.zeros(n + 16, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 16:][:n]
    d, counts, totals = torch.ones(4, 3), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_expose(d, 1, 0, 1, 1, 2, 8, ws, counts, totals)
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    for call in (lambda: mesh.mesh_exposure(v, t), lambda: mesh.cull_hidden(v, t)):
        with pytest.raises(pvd_hip.PvdHipError):
            call()
    for bad in (dict(mode="faces"), dict(sides="back")):
        with pytest.raises(ValueError):
            mesh.cull_hidden(v, t, **bad)
    sig = inspect.signature(mesh.cull_hidden).parameters
    assert (sig["mode"].default, sig["sides"].default, sig["min_escaped"].default, sig["samples"].default) == ("shells", "front", 1, 1)
    sig = inspect.signature(mesh.mesh_exposure).parameters
    assert sig["dirs"].default is None and sig["samples"].default == 1 and sig["band"].default is None and sig["return_totals"].default is False


def test_the_default_directions():
    import numpy as np
    import mesh_expose_restatement as er
    from pvd.mesh import exposure_directions
    d = exposure_directions(64)
    assert d.dtype.is_floating_point and tuple(d.shape) == (64, 3) and d.numpy().dtype == np.float32
    assert d.numpy().tobytes() == er.directions(64).tobytes() == exposure_directions(64).numpy().tobytes()
    assert np.all(d.numpy() != 0) and np.all(er.valid_directions(d.numpy()))  # none along an axis or in a lattice plane
    assert np.allclose(np.linalg.norm(d.numpy().astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert abs(d.numpy().astype(np.float64).mean(axis=0)).max() < 0.02  # spread over the sphere
    assert tuple(exposure_directions(1).shape) == (1, 3) and tuple(exposure_directions(1024).shape) == (1024, 3)
