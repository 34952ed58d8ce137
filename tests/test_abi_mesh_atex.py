"""csrc/pvd_hip_mesh_atex.h -- the area-adaptive texture atlas -- next to the other mesh headers: the new header declares exactly five
names and five constants, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the headers of include/, their
lists and the ABI number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import inspect
import os
import re

import pytest

import mesh_atex_restatement as ar

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "aaai2023-pvd_amd", "csrc")
NAMES = ["pvd_mesh_atex_build", "pvd_mesh_atex_layout", "pvd_mesh_atex_points", "pvd_mesh_atex_sample", "pvd_mesh_atex_workspace_bytes"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip_mesh_ray.h": "ENTRY_POINTS_MESH_RAY",
          "pvd_hip_mesh_smooth.h": "ENTRY_POINTS_MESH_SMOOTH", "pvd_hip_mesh_topo.h": "ENTRY_POINTS_MESH_TOPO",
          "pvd_hip_mesh_winding.h": "ENTRY_POINTS_MESH_WINDING", "pvd_hip_mesh_tex.h": "ENTRY_POINTS_MESH_TEX",
          "pvd_hip_prefix.h": "ENTRY_POINTS_PREFIX", "pvd_hip.h": "ENTRY_POINTS"}
CSRC_TUPLES = ("ENTRY_POINTS_MESH_EXPOSE", "ENTRY_POINTS_MESH_SHTEX", "ENTRY_POINTS_MESH_TSDF", "ENTRY_POINTS_MESH_PROJECT")
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _include(header):
    return os.path.join(REPO, "include", header)


def test_the_header_declares_exactly_the_five_names_and_the_constants():
    path = os.path.join(CSRC, "pvd_hip_mesh_atex.h")
    assert _declared(path) == NAMES
    src = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert dict(re.findall(r"^#define (PVD_MESH_ATEX_[A-Z_]+) (\S+)", code, flags=re.M)) == {
        "PVD_MESH_ATEX_CLASSES": "5", "PVD_MESH_ATEX_MAX_T": "268435455", "PVD_MESH_ATEX_MAX_SIDE": "16384", "PVD_MESH_ATEX_TOTALS": "6",
        "PVD_MESH_ATEX_LAYOUT_WORDS": "17"}
    assert '#include "../../include/pvd_hip_mesh_tex.h"' in code
    # the definition is in the header, operation by operation
    assert "NOTHING IS FUSED" in src and "NOT FROM ATOMICS" in src
    for line in ("S_c = 4, 8, 16, 32, 64", "m_c = S_c - 3 = 1, 5, 13, 29, 61",
                 "dAB = ((ux*ux + uy*uy) + uz*uz) with u = B - A",
                 "L2 = fmaxf(fmaxf(dAB, dAC), dBC)",
                 "q = L2 * rho2,   rho2 = density * density",
                 "c0 = the number of i in 0 .. 3 with q > (float)(m_i * m_i)",
                 "the thresholds 1, 25, 169, 841",
                 "c = min(c0, max_class)",
                 "CAPPED when c0 > max_class or q > 3721",
                 "has class 0\n *          and is not capped",
                 "m_c >= density * (its longest edge)",
                 "slot[f]  u32 = c << 28 | rank",
                 "order[base_c + rank] u32 = f",
                 "totals[6] u32 = count_0 .. count_4, the number of capped triangles",
                 "cells_c = ceil(count_c / 2);   A = sum of cells_c * S_c * S_c",
                 "Wt = the smallest multiple of 64 with Wt * Wt >= A, and at least 64",
                 "C_c = Wt / S_c cells per row, rows_c = ceil(cells_c / C_c)",
                 "T = 0 gives Wt = 64, Ht = 4, with nothing owned",
                 "beta = (float)p / (float)m_c,   gamma = (float)q / (float)m_c,   alpha = (1 - beta) - gamma",
                 "ranks 2k and 2k + 1 share cell k",
                 "uv = (X / Wt, 1 - Y / Ht)",
                 "WHY NO GUTTER IS NEEDED holds per cell",
                 "rank - 1 of ITS CLASS",
                 "c = (c00 * (1 - tx) + c10 * tx) * (1 - ty) + (c01 * (1 - tx) + c11 * tx) * ty",
                 "Every read stays inside the triangle's own cell, whatever bary holds"):
        assert line in src, line
    assert src.count("before any device call") >= 3  # build, points, sample


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared(_include("pvd_hip.h"))) == 75
    assert len(_declared(_include("pvd_hip_mesh_tex.h"))) == 3
    assert set(OTHERS) == set(os.listdir(os.path.join(REPO, "include")))
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(_include(h))), h
        assert "PVD_MESH_ATEX_" not in open(_include(h)).read(), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_ATEX, tuple) and sorted(pvd_hip.ENTRY_POINTS_MESH_ATEX) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(_include(header)), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_ATEX) & set(getattr(pvd_hip, tup)), header
    for tup in CSRC_TUPLES:
        assert not set(pvd_hip.ENTRY_POINTS_MESH_ATEX) & set(getattr(pvd_hip, tup)), tup
    for name in NAMES:
        assert callable(getattr(pvd_hip, name[len("pvd_"):]))
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_ATEX_CELLS == (4, 8, 16, 32, 64) == ar.CELLS
    assert pvd_hip.MESH_ATEX_TOTALS == ("count_0", "count_1", "count_2", "count_3", "count_4", "capped") == ar.TOTALS
    assert pvd_hip.MESH_ATEX_MAX_T == ar.MAX_T == 2 ** 28 - 1 and pvd_hip.MESH_ATEX_MAX_SIDE == ar.MAX_SIDE == 16384


def test_the_source_and_the_header_are_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert "mesh_atex.hip" in srcs and " pvd_hip_mesh_atex.h " in mk and " block_scan.h " in mk and " mesh_atlas.h " in mk
    assert "-ffp-contract=off" in [ln for ln in mk.splitlines() if ln.startswith("FLAGS")][0]
    src = open(os.path.join(CSRC, "mesh_atex.hip")).read()
    assert '#include "pvd_hip_mesh_atex.h"' in src and '#include "block_scan.h"' in src and '#include "mesh_atlas.h"' in src
    assert "#pragma clang fp contract(off)" in src and "fma(" not in src and "fmaf(" not in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code  # the ranks come from scans
    assert "scan_sums(" in code and "block_exclusive(" in code and "block_sum(" in code
    assert "footprint_of(" in code and "blend(" in code and "texel_point(" in code  # the per-cell arithmetic is csrc/mesh_atlas.h's, shared
    tex = open(os.path.join(CSRC, "mesh_tex.hip")).read()
    assert "texel_point(" in tex and "float mix3(" not in tex and "float mix3(" in open(os.path.join(CSRC, "mesh_atlas.h")).read()


@pytest.mark.parametrize("counts", [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 0, 7, 0, 0), (0, 0, 0, 0, 1), (1, 0, 0, 0, 1), (5, 0, 3, 0, 2),
                                    (33, 17, 9, 5, 3), (100000, 30000, 8000, 900, 50), (0, 0, 0, 0, 2 * 256 * 256)])
def test_the_layout_equals_the_restatement(hip_lib_built, counts):
    import pvd_hip
    Wt, Ht, y0, rows, C = pvd_hip.mesh_atex_layout(counts)
    assert [Wt, Ht] + list(y0) + list(rows) + list(C) == ar.layout_words(counts)


def test_the_layout_refuses_a_side_above_16384_and_null_pointers(hip_lib_built):
    import pvd_hip
    lib = ctypes.CDLL(hip_lib_built)
    lib.pvd_mesh_atex_layout.restype = ctypes.c_int
    out = (ctypes.c_uint32 * 17)(*([77] * 17))
    for bad in ((0, 0, 0, 0, 2 * 256 * 256 + 1), (1, 0, 0, 0, 2 * 256 * 256), (2 ** 28, 0, 0, 0, 0), (2 ** 32 - 1,) * 5):
        assert lib.pvd_mesh_atex_layout((ctypes.c_uint32 * 5)(*bad), out) == UNSUPPORTED, bad
        assert list(out) == [77] * 17  # not written
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_atex_layout(bad)
        with pytest.raises(ValueError):
            ar.layout(bad)
    good = (ctypes.c_uint32 * 5)(1, 2, 3, 4, 5)
    assert lib.pvd_mesh_atex_layout(None, out) == INVALID and lib.pvd_mesh_atex_layout(good, None) == INVALID
    assert lib.pvd_mesh_atex_layout(good, out) == OK and list(out) == ar.layout_words((1, 2, 3, 4, 5))


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """Unsupported first (T above 2^28 - 1, max_class above 4; for points and sample the layout's limits, after NULL counts); then a
    density that is not positive or whose square is not a positive finite float32; then counts that do not sum to T and rows outside the
    atlas; then nothing to do: PVD_OK with no launch, NULL pointers allowed; then NULL pointers and a bad workspace: PVD_ERR_INVALID --
    all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp, sz = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    one, null = vp(64), vp(0)
    for name in NAMES:
        getattr(lib, name).restype = ctypes.c_int
    lib.pvd_mesh_atex_workspace_bytes.restype = ctypes.c_size_t
    inf, nan = float("inf"), float("nan")
    wsb = lib.pvd_mesh_atex_workspace_bytes
    assert wsb(u32(0)) == 16 and wsb(u32(1)) == 32 and wsb(u32(256)) == 32 and wsb(u32(257)) == 48 and wsb(u32(2 ** 28 - 1)) == 6 * 4 * 2 ** 20
    assert wsb(u32(2 ** 28)) == 0 and wsb(u32(2 ** 32 - 1)) == 0
    T = 300
    need = wsb(u32(T))

    def build(vertices=one, V=9, triangles=one, T=T, density=20.0, max_class=4, ws=one, ws_bytes=need, slot=one, order=one, totals=one):
        return lib.pvd_mesh_atex_build(vertices, u32(V), triangles, u32(T), f32(density), u32(max_class), ws, sz(ws_bytes), slot, order, totals,
                                       null)
    # (no call below passes every check with work to do: none reaches a launch)
    assert build(T=2 ** 28) == UNSUPPORTED and build(max_class=5) == UNSUPPORTED and build(max_class=5, density=nan) == UNSUPPORTED
    for bad in (0.0, -1.0, nan, inf, -inf, 1e30, 1e-30):
        assert build(density=bad) == INVALID and build(density=bad, totals=null) == INVALID, bad
    assert build(totals=null) == INVALID and build(totals=null, T=0) == INVALID
    for k in ("vertices", "triangles", "slot", "order", "ws"):
        assert build(**{k: null}) == INVALID, k
    assert build(ws=vp(72)) == INVALID and build(ws_bytes=need - 1) == INVALID

    def counts_of(*c):
        return (ctypes.c_uint32 * 5)(*c)
    good = counts_of(100, 100, 50, 40, 10)  # sums to T; 128 x 124... whatever the layout says
    Ht = ar.layout((100, 100, 50, 40, 10))["Ht"]
    huge = counts_of(0, 0, 0, 0, 2 * 256 * 256 + 1)

    def points(vertices=one, V=9, triangles=one, T=T, normals=one, counts=good, order=one, row0=0, row1=Ht, x=one, n=one):
        return lib.pvd_mesh_atex_points(vertices, u32(V), triangles, u32(T), normals, counts, order, u32(row0), u32(row1), x, n, null)
    assert points(counts=None) == INVALID and points(counts=huge) == UNSUPPORTED and points(counts=huge, T=2 * 256 * 256 + 1) == UNSUPPORTED
    assert points(T=T + 1) == INVALID and points(T=T - 1) == INVALID and points(T=T + 1, row1=0) == INVALID
    assert points(row0=2, row1=1) == INVALID and points(row1=Ht + 1) == INVALID
    nulls = dict(vertices=null, triangles=null, normals=null, order=null, x=null, n=null)
    assert points(row0=3, row1=3) == OK and points(row0=0, row1=0, **nulls) == OK and points(row0=Ht, row1=Ht, **nulls) == OK
    for k in ("vertices", "triangles", "order", "x", "n"):
        assert points(**{k: null}) == INVALID, k

    def sample(texture=one, T=T, counts=good, slot=one, tri=one, bary=one, N=5, bg3=one, color=one):
        return lib.pvd_mesh_atex_sample(texture, u32(T), counts, slot, tri, bary, u32(N), bg3, color, null)
    assert sample(counts=None) == INVALID and sample(counts=huge) == UNSUPPORTED and sample(counts=huge, N=0) == UNSUPPORTED
    assert sample(T=T + 1) == INVALID and sample(T=T + 1, N=0) == INVALID
    assert sample(N=0) == OK and sample(N=0, texture=null, slot=null, tri=null, bary=null, bg3=null, color=null) == OK
    for k in ("texture", "slot", "tri", "bary", "bg3", "color"):
        assert sample(**{k: null}) == INVALID, k


def test_the_binding_rejects_cpu_tensors_and_wrong_arguments(hip_lib_built):
    import torch
    import pvd_hip
    from pvd import mesh
    z = torch.zeros
    i32 = dict(dtype=torch.int32)
    ws = z(4096, dtype=torch.uint8)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_atex_build(z(6, 3), z(2, 3, **i32), 20.0, 4, ws, z(2, **i32), z(2, **i32), z(6, **i32))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_atex_points(z(6, 3), z(2, 3, **i32), None, (2, 0, 0, 0, 0), z(2, **i32), 0, 4, z(4 * 64, 3), z(4 * 64, 3))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_atex_sample(z(4, 64, 3), 2, (2, 0, 0, 0, 0), z(2, **i32), z(5, **i32), z(5, 2), z(3), z(5, 3))
    for bad in ((1, 2, 3), (1, 0, 0, 0, -1), (2 ** 32, 0, 0, 0, 0)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_atex_layout(bad)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_atex_workspace_bytes(2 ** 28)
    assert pvd_hip.mesh_atex_workspace_bytes(0) == 16
    sig = inspect.signature(mesh.adaptive_atlas).parameters
    assert list(sig) == ["vertices", "triangles", "density", "max_cell"] and sig["max_cell"].default == 64
    for bad in (dict(density=0.0), dict(density=-1.0), dict(density=float("nan")), dict(density=20.0, max_cell=12)):
        with pytest.raises(ValueError):
            mesh.adaptive_atlas(z(6, 3), z(2, 3, **i32), **bad)
    # the existing signatures keep their parameters and defaults; the new switch is off by default
    assert list(inspect.signature(mesh.bake_texture).parameters) == ["source", "vertices", "triangles", "S", "normals", "chunk"]
    assert list(inspect.signature(mesh.sample_texture).parameters) == ["texture", "S", "T", "tri", "bary", "bg_color"]
    for fn in (mesh.extract_surface, mesh.extract_surface_tsdf):
        sig = inspect.signature(fn).parameters
        assert sig["texture"].default == 0 and sig["texture_sh"].default == 0 and sig["texture_density"].default == 0.0
    # an adaptive atlas where an SH atlas needs an integer: ValueError, before anything is computed
    atlas = dict(slot=z(2, **i32), order=z(2, **i32), counts=(2, 0, 0, 0, 0), triangles=2)
    with pytest.raises(ValueError):
        mesh.bake_sh_texture(lambda x, d: x, z(6, 3), z(2, 3, **i32), atlas)
    with pytest.raises(ValueError):
        mesh.sample_sh_texture(z(4, 64, 4, 3), atlas, 2, z(5, **i32), z(5, 2), z(5, 3))
