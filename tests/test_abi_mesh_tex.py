"""include/pvd_hip_mesh_tex.h -- texture atlases -- next to the other mesh headers: the new header declares exactly three names and three
constants, libpvd_hip.so exports them, the binding lists them in a tuple of its own, and the other headers, their lists and the ABI
number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["pvd_mesh_tex_layout", "pvd_mesh_tex_points", "pvd_mesh_tex_sample"]
DEFINES = {"PVD_MESH_TEX_MIN_S": "4", "PVD_MESH_TEX_MAX_S": "64", "PVD_MESH_TEX_MAX_SIDE": "16384"}
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip_mesh_ray.h": "ENTRY_POINTS_MESH_RAY",
          "pvd_hip_mesh_smooth.h": "ENTRY_POINTS_MESH_SMOOTH", "pvd_hip_mesh_topo.h": "ENTRY_POINTS_MESH_TOPO",
          "pvd_hip_mesh_winding.h": "ENTRY_POINTS_MESH_WINDING", "pvd_hip_prefix.h": "ENTRY_POINTS_PREFIX", "pvd_hip.h": "ENTRY_POINTS"}
SIZES = tuple(range(4, 10))
COUNTS = (0, 1, 2, 7, 50)


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_header_declares_exactly_the_three_entry_points_and_the_three_constants():
    assert _declared("pvd_hip_mesh_tex.h") == NAMES
    src = _source("pvd_hip_mesh_tex.h")
    assert '#include "pvd_hip.h"' in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = dict(re.findall(r"^#define (PVD_MESH_TEX_[A-Z_]+) (\S+)$", code, flags=re.M))
    assert found == DEFINES
    assert sorted(set(re.findall(r"^#define (\w+)", code, flags=re.M))) == sorted(list(DEFINES) + ["PVD_HIP_MESH_TEX_H"])
    # the definition is in the header: the weights, the point, why no gutter is needed, what the layout costs
    assert "NOTHING IS FUSED" in src and "alpha = (1 - beta) - gamma" in src and "X = (alpha * A + beta * B) + gamma * Cc" in src
    assert "c = (c00 * (1 - tx) + c10 * tx) * (1 - ty) + (c01 * (1 - tx) + c11 * tx) * ty" in src
    assert "NO GUTTER PASS IS NEEDED" in src and "39 % at S = 8, 66 % at S = 16" in src and "ONE TEXEL DENSITY SERVES ALL TRIANGLES" in src
    assert "uv = (X / Wt, 1 - Y / Ht)" in src and "six NaNs" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh_ray.h") == ["pvd_mesh_ray_build", "pvd_mesh_ray_cast", "pvd_mesh_ray_count", "pvd_mesh_ray_workspace_bytes"]
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h != "pvd_hip_mesh_tex.h":
            assert not set(NAMES) & set(_declared(h)), h
            assert "PVD_MESH_TEX_" not in _source(h), h
    assert set(OTHERS) | {"pvd_hip_mesh_tex.h"} == set(os.listdir(os.path.join(REPO, "include")))
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_TEX, tuple) and sorted(pvd_hip.ENTRY_POINTS_MESH_TEX) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(header), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_TEX) & set(getattr(pvd_hip, tup)), header
    for name in NAMES:
        assert callable(getattr(pvd_hip, name[4:])), name
    assert pvd_hip.ABI_VERSION == 6
    assert (pvd_hip.MESH_TEX_MIN_S, pvd_hip.MESH_TEX_MAX_S, pvd_hip.MESH_TEX_MAX_SIDE) == (4, 64, 16384)
    import mesh_tex_restatement as tr
    assert (tr.MIN_S, tr.MAX_S, tr.MAX_SIDE) == (4, 64, 16384)


def test_the_source_and_the_header_are_in_the_makefile():
    mk = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    assert "mesh_tex.hip" in srcs.split() and "../../include/pvd_hip_mesh_tex.h" in mk
    assert "-ffp-contract=off" in [ln for ln in mk.splitlines() if ln.startswith("FLAGS")][0]
    src = open(os.path.join(REPO, "aaai2023-pvd_amd", "csrc", "mesh_tex.hip")).read()
    assert "fma(" not in src and "fmaf(" not in src and "__shared__" not in src and "atomic" not in src.replace("no atomics", "")


@pytest.mark.parametrize("S", SIZES)
def test_the_layout_agrees_with_the_restatement(S, hip_lib_built):
    import mesh_tex_restatement as tr
    import pvd_hip
    from pvd.mesh import texture_layout
    for T in COUNTS + (3, 51, 659256):
        assert pvd_hip.mesh_tex_layout(T, S) == tr.layout(T, S), (T, S)
        C, rows, Wt, Ht = tr.layout(T, S)
        assert texture_layout(T, S) == dict(cells_per_row=C, rows=rows, width=Wt, height=Ht, cell=S, triangles=T)


def test_the_layout_refuses_a_cell_of_3_or_65_and_a_side_above_16384(hip_lib_built):
    import mesh_tex_restatement as tr
    import pvd_hip
    lib = ctypes.CDLL(hip_lib_built)
    lib.pvd_mesh_tex_layout.restype = ctypes.c_int
    u32 = ctypes.c_uint32
    out = (u32 * 4)(7, 7, 7, 7)
    for T, S in ((5, 3), (5, 65), (5, 0), (2 * 4096 * 4096 + 1, 4), (2 * 256 * 256 + 1, 64), (2 ** 32 - 1, 4), (2 * 1024 * 1024 + 1, 16)):
        assert lib.pvd_mesh_tex_layout(u32(T), u32(S), out) == -2 and list(out) == [7, 7, 7, 7], (T, S)
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_tex_layout(T, S)
        with pytest.raises(ValueError):
            tr.layout(T, S)
    for T, S in ((2 * 4096 * 4096, 4), (2 * 256 * 256, 64), (2 * 1024 * 1024, 16)):  # the largest that fit
        assert lib.pvd_mesh_tex_layout(u32(T), u32(S), out) == 0 and tuple(out) == tr.layout(T, S) and out[2] == 16384 and out[3] == 16384
    assert lib.pvd_mesh_tex_layout(u32(5), u32(8), ctypes.c_void_p(0)) == -1
    for bad in ((-1, 8), (2 ** 32, 8), (5, -1), (5, 2 ** 32)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_tex_layout(*bad)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """The layout's errors (PVD_ERR_UNSUPPORTED) first; rows outside 0 <= row0 <= row1 <= Ht: PVD_ERR_INVALID; an empty band or N == 0:
    PVD_OK with no launch, NULL pointers allowed; then NULL pointers: PVD_ERR_INVALID -- all before a device is touched (the pointers are
    never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    one = vp(64)
    for name in NAMES:
        getattr(lib, name).restype = ctypes.c_int

    def points(verts=one, V=9, tris=one, T=5, normals=vp(0), S=8, row0=0, row1=0, x=one, n=one):
        return lib.pvd_mesh_tex_points(verts, u32(V), tris, u32(T), normals, u32(S), u32(row0), u32(row1), x, n, vp(0))
    assert points(S=3) == -2 and points(S=65) == -2 and points(T=2 * 4096 * 4096 + 1, S=4) == -2
    assert points(S=3, row0=5, row1=2) == -2  # the layout first
    assert points(row0=5, row1=2) == -1 and points(row0=0, row1=17) == -1 and points(row0=17, row1=17) == -1  # Ht = 16 for T = 5, S = 8
    assert points(row0=16, row1=16) == 0 and points(row0=3, row1=3, verts=vp(0), tris=vp(0), x=vp(0), n=vp(0)) == 0
    assert points(row1=1, verts=vp(0)) == -1 and points(row1=1, tris=vp(0)) == -1 and points(row1=1, x=vp(0)) == -1
    assert points(row1=1, n=vp(0)) == -1

    def sample(tex=one, T=5, S=8, tri=one, bary=one, N=0, bg=one, color=one):
        return lib.pvd_mesh_tex_sample(tex, u32(T), u32(S), tri, bary, u32(N), bg, color, vp(0))
    assert sample(S=3) == -2 and sample(S=65, N=4) == -2 and sample(T=2 * 4096 * 4096 + 1, S=4) == -2
    assert sample() == 0 and sample(tex=vp(0), tri=vp(0), bary=vp(0), bg=vp(0), color=vp(0)) == 0
    assert sample(N=4, tex=vp(0)) == -1 and sample(N=4, tri=vp(0)) == -1 and sample(N=4, bary=vp(0)) == -1
    assert sample(N=4, bg=vp(0)) == -1 and sample(N=4, color=vp(0)) == -1


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import inspect

    import torch
    import pvd_hip
    from pvd import mesh
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    x, n = torch.zeros(16, 3), torch.zeros(16, 3)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_tex_points(v, t, None, 4, 0, 4, x, n)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_tex_sample(torch.zeros(4, 4, 3), 1, 4, torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2), torch.zeros(3), torch.zeros(2, 3))
    for call in (lambda: mesh.texture_points(v, t, 4), lambda: mesh.sample_texture(torch.zeros(4, 4, 3), 4, 1, t[:, 0], torch.zeros(1, 2)),
                 lambda: mesh.bake_texture(lambda a, b: a, v, t, 4)):
        with pytest.raises(pvd_hip.PvdHipError):
            call()
    # the new arguments are off unless asked for
    for fn, name, default in ((mesh.render_mesh, "texture", None), (mesh.render_mesh, "texture_cell", None),
                              (mesh.evaluate_mesh_views, "texture", None), (mesh.evaluate_mesh_views, "texture_cell", None),
                              (mesh.extract_surface, "texture", 0)):
        assert inspect.signature(fn).parameters[name].default == default or inspect.signature(fn).parameters[name].default is default
