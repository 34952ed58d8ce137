"""csrc/pvd_hip_mesh_project.h -- the projection of posed images onto surface points -- next to the other mesh headers: the new header
declares exactly two names and six constants, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the
headers of include/, their lists and the ABI number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles
gfx950 on CPU)."""
import ctypes
import inspect
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "aaai2023-pvd_amd", "csrc")
NAMES = ["pvd_mesh_project_finalize", "pvd_mesh_project_integrate"]
OTHERS = {"pvd_hip_mlp.h": "ENTRY_POINTS_MLP", "pvd_hip_metrics.h": "ENTRY_POINTS_METRICS", "pvd_hip_data.h": "ENTRY_POINTS_DATA",
          "pvd_hip_march.h": "ENTRY_POINTS_MARCH", "pvd_hip_mesh.h": "ENTRY_POINTS_MESH", "pvd_hip_components.h": "ENTRY_POINTS_COMPONENTS",
          "pvd_hip_mesh_attr.h": "ENTRY_POINTS_MESH_ATTR", "pvd_hip_mesh_dist.h": "ENTRY_POINTS_MESH_DIST",
          "pvd_hip_mesh_simplify.h": "ENTRY_POINTS_MESH_SIMPLIFY", "pvd_hip_mesh_ray.h": "ENTRY_POINTS_MESH_RAY",
          "pvd_hip_mesh_smooth.h": "ENTRY_POINTS_MESH_SMOOTH", "pvd_hip_mesh_topo.h": "ENTRY_POINTS_MESH_TOPO",
          "pvd_hip_mesh_winding.h": "ENTRY_POINTS_MESH_WINDING", "pvd_hip_mesh_tex.h": "ENTRY_POINTS_MESH_TEX",
          "pvd_hip_prefix.h": "ENTRY_POINTS_PREFIX", "pvd_hip.h": "ENTRY_POINTS"}
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def _include(header):
    return os.path.join(REPO, "include", header)


def test_the_header_declares_exactly_the_two_names_and_the_constants():
    path = os.path.join(CSRC, "pvd_hip_mesh_project.h")
    assert _declared(path) == NAMES
    src = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert dict(re.findall(r"^#define (PVD_MESH_PROJECT_[A-Z_]+) (\S+)$", code, flags=re.M)) == {
        "PVD_MESH_PROJECT_MAX_SIDE": "16384", "PVD_MESH_PROJECT_MAX_POWER": "8", "PVD_MESH_PROJECT_SIDES_FRONT": "0",
        "PVD_MESH_PROJECT_SIDES_BOTH": "1", "PVD_MESH_PROJECT_MODE_BLEND": "0", "PVD_MESH_PROJECT_MODE_BEST": "1"}
    assert '#include "../../include/pvd_hip_mesh_ray.h"' in code
    # the definition is in the header, operation by operation
    assert "NOTHING IS FUSED" in src and "EVERY NaN SKIPS" in src
    for line in ("L = sqrtf((n_x * n_x + n_y * n_y) + n_z * n_z)",
                 "e = o - p",
                 "r = sqrtf((e_x * e_x + e_y * e_y) + e_z * e_z);    r > 0, or the view is skipped",
                 "c = ((u_x * e_x + u_y * e_y) + u_z * e_z) / r",
                 "s = -1 if c < 0 and s = 1 otherwise, then c = |c|",
                 "c > cos_min, or the view is skipped",
                 "q_a = (M[0][a] * d_x + M[1][a] * d_y) + M[2][a] * d_z",
                 "q_z > 0, or the view is skipped",
                 "x = (fx * q_x) / q_z + cx,      y = (fy * q_y) / q_z + cy",
                 "0.5 <= x <= W - 0.5 and 0.5 <= y <= H - 0.5, or the view is skipped",
                 "a = x - 0.5;   i = min((int)floorf(a), W - 2);   f = a - (float)i",
                 "m00 = (1 - f) * (1 - g),   m10 = f * (1 - g),   m01 = (1 - f) * g,   m11 = f * g",
                 "C_ch = ((m00 * I00 + m10 * I10) + m01 * I01) + m11 * I11",
                 "all twelve values I must be finite",
                 "0 < wp < +inf, or the view is skipped",
                 "w = 1;   w = w * c, `power` times",
                 "o'_a = p_a + (s * bias) * u_a",
                 "D_a = (double)o_a - (double)o'_a",
                 "0 <= t < 1",
                 "acc_w = acc_w + w;   acc_c[ch] = acc_c[ch] + w * C_ch",
                 "if w > acc_w:  acc_w = w and acc_c = C",
                 "colors[ch] = fminf(fmaxf(acc_c[ch] / acc_w, 0), 1)",
                 "colors[ch] = fminf(fmaxf(acc_c[ch], 0), 1)"):
        assert line in src, line
    assert "THE POINT OF THE TRIANGLE" in src and "pvd_hip_mesh_expose.h" in src  # the edge-on exception is named
    assert "views can arrive in batches" in src and "ties keep the earlier view" in src and "LEFT AS THE CALLER FILLED IT" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared(_include("pvd_hip.h"))) == 75
    assert set(OTHERS) == set(os.listdir(os.path.join(REPO, "include")))
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(_include(h))), h
        assert "PVD_MESH_PROJECT_" not in open(_include(h)).read(), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_PROJECT, tuple) and sorted(pvd_hip.ENTRY_POINTS_MESH_PROJECT) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(_include(header)), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_PROJECT) & set(getattr(pvd_hip, tup)), header
    assert not set(pvd_hip.ENTRY_POINTS_MESH_PROJECT) & (set(pvd_hip.ENTRY_POINTS_MESH_EXPOSE) | set(pvd_hip.ENTRY_POINTS_MESH_SHTEX)
                                                         | set(pvd_hip.ENTRY_POINTS_MESH_TSDF))
    for name in NAMES:
        assert callable(getattr(pvd_hip, name[len("pvd_"):]))
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_PROJECT_MAX_SIDE == 16384 and pvd_hip.MESH_PROJECT_MAX_POWER == 8
    assert pvd_hip.MESH_PROJECT_SIDES == ("front", "both") and pvd_hip.MESH_PROJECT_MODES == ("blend", "best")
    assert pvd_hip.MESH_PROJECT_TOTALS == ("seen", "unseen")
    import mesh_project_restatement as pr
    assert pr.MAX_SIDE == 16384 and pr.MAX_POWER == 8 and pr.SIDES == pvd_hip.MESH_PROJECT_SIDES and pr.MODES == pvd_hip.MESH_PROJECT_MODES
    assert pr.TOTALS == pvd_hip.MESH_PROJECT_TOTALS


def test_the_source_and_the_header_are_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert "mesh_project.hip" in srcs and " pvd_hip_mesh_project.h " in mk
    assert "-ffp-contract=off" in [ln for ln in mk.splitlines() if ln.startswith("FLAGS")][0]
    src = open(os.path.join(CSRC, "mesh_project.hip")).read()
    assert '#include "pvd_hip_mesh_project.h"' in src and '#include "mesh_ray_walk.h"' in src and "#pragma clang fp contract(off)" in src
    assert "fma(" not in src and "fmaf(" not in src and "__shared__" not in src
    kernel = src[src.index("void k_mp_integrate"):src.index("void k_mp_finalize")]
    assert "atomic" not in kernel and "walk(" in kernel  # the integration: the shared walk, no atomics
    assert "atomicAdd(&totals" in src and "__ballot" in src  # the totals of the finalize pass: integer atomics per wave


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """Unsupported first (W or H outside 2 .. 16384, power above 8, an unknown sides or mode); then cos_min outside [0, 1) or NaN, then a
    bias that is negative or not finite (min_weight not positive or not finite for finalize): PVD_ERR_INVALID; then the workspace
    checks of pvd_mesh_ray_build; then nothing to do (N or V of 0): PVD_OK with no launch, NULL pointers allowed; then NULL pointers:
    PVD_ERR_INVALID -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, u64, f32, vp, sz = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    one, null = vp(64), vp(0)
    for name in NAMES:
        getattr(lib, name).restype = ctypes.c_int
    lib.pvd_mesh_ray_workspace_bytes.restype = ctypes.c_size_t
    inf, nan = float("inf"), float("nan")
    T, G, PAIRS = 12, 4, 40
    need = lib.pvd_mesh_ray_workspace_bytes(u32(T), u32(G), u64(PAIRS))
    assert need > 0

    def integrate(points=one, normals=one, N=5, color=one, weight=one, poses=one, intr=one, V=3, H=5, W=7, T=T, G=G, pairs=PAIRS, ws=one,
                  ws_bytes=need, cos_min=0.2, power=2, bias=0.001, sides=0, mode=0, acc_c=one, acc_w=one):
        return lib.pvd_mesh_project_integrate(points, normals, u32(N), color, weight, poses, intr, u32(V), u32(H), u32(W), u32(T), u32(G),
                                              u64(pairs), ws, sz(ws_bytes), f32(cos_min), u32(power), f32(bias), u32(sides), u32(mode), acc_c,
                                              acc_w, null)
    # (no call below passes every check: none reaches a launch)
    for k in ("H", "W"):
        for bad in (0, 1, 16385):
            assert integrate(**{k: bad}) == UNSUPPORTED and integrate(**{k: bad}, N=0) == UNSUPPORTED, (k, bad)
    assert integrate(power=9) == UNSUPPORTED and integrate(sides=2) == UNSUPPORTED and integrate(mode=2) == UNSUPPORTED
    assert integrate(power=9, cos_min=nan) == UNSUPPORTED  # unsupported comes first
    for bad in (-0.1, 1.0, 2.0, nan, inf):
        assert integrate(cos_min=bad) == INVALID and integrate(cos_min=bad, V=0) == INVALID, bad
    for bad in (-1.0, inf, nan):
        assert integrate(bias=bad) == INVALID and integrate(bias=bad, N=0) == INVALID, bad
    assert integrate(bias=nan, ws=null) == INVALID and integrate(bias=nan, G=0) == INVALID  # the bias comes before the workspace
    # the workspace checks of pvd_mesh_ray_build: NULL, unaligned or short: invalid; G, T or pairs out of range: unsupported
    assert integrate(ws=null, N=0) == INVALID and integrate(ws=vp(72), N=0) == INVALID and integrate(ws_bytes=need - 1, N=0) == INVALID
    assert integrate(G=0, N=0) == UNSUPPORTED and integrate(G=257, N=0) == UNSUPPORTED and integrate(pairs=2 ** 31, N=0) == UNSUPPORTED
    # nothing to do: OK, and no pointer is read
    nulls = dict(points=null, normals=null, color=null, weight=null, poses=null, intr=null, acc_c=null, acc_w=null)
    assert integrate(N=0) == OK and integrate(V=0) == OK and integrate(N=0, **nulls) == OK and integrate(V=0, **nulls) == OK
    assert integrate(N=0, power=0, bias=0.0, cos_min=0.0, sides=1, mode=1) == OK
    for k in ("points", "normals", "color", "poses", "intr", "acc_c", "acc_w"):
        assert integrate(**{k: null}) == INVALID, k

    def finalize(acc_c=one, acc_w=one, N=5, min_weight=1.0, mode=0, colors=one, seen=one, totals=one):
        return lib.pvd_mesh_project_finalize(acc_c, acc_w, u32(N), f32(min_weight), u32(mode), colors, seen, totals, null)
    assert finalize(mode=2) == UNSUPPORTED and finalize(mode=2, min_weight=nan) == UNSUPPORTED and finalize(mode=7, N=0) == UNSUPPORTED
    for bad in (0.0, -1.0, inf, nan):
        assert finalize(min_weight=bad) == INVALID and finalize(min_weight=bad, N=0) == INVALID, bad
    assert finalize(N=0) == OK and finalize(N=0, acc_c=null, acc_w=null, colors=null, seen=null, totals=null) == OK
    assert finalize(N=0, mode=1) == OK
    for k in ("acc_c", "acc_w", "colors", "seen", "totals"):
        assert finalize(**{k: null}) == INVALID, k


def test_the_binding_rejects_cpu_tensors_and_wrong_arguments(hip_lib_built):
    import torch
    import pvd_hip
    from pvd import mesh
    z = torch.zeros
    ws = z(4096, dtype=torch.uint8)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_project_integrate(z(4, 3), z(4, 3), z(1, 5, 7, 3), None, z(1, 4, 4), z(1, 4), 0, 1, 0, ws, 0.2, 2, 0.0, "front", "blend",
                                       z(4, 3), z(4))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_project_finalize(z(4, 3), z(4), 1.0, "blend", z(4, 3), z(4, dtype=torch.uint8), z(2, dtype=torch.int64))
    sig = inspect.signature(mesh.project_views).parameters
    assert list(sig)[:7] == ["points", "normals", "vertices", "triangles", "color", "poses", "intrinsics"]
    assert [sig[k].default for k in ("weight", "cos_min", "power", "bias", "sides", "mode", "fallback", "views_per_batch", "grid")] == \
        [None, 0.2, 2, None, "front", "blend", None, 16, None]
    assert 0 < sig["min_weight"].default < 1e-3
    assert list(inspect.signature(mesh.view_source).parameters)[:6] == ["vertices", "triangles", "color", "poses", "intrinsics", "fallback"]
    assert callable(mesh.view_vertex_colors)
    # the existing signatures keep their defaults
    sig = inspect.signature(mesh.bake_texture).parameters
    assert list(sig) == ["source", "vertices", "triangles", "S", "normals", "chunk"]
