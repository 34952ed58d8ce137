"""csrc/pvd_hip_mesh_tsdf.h -- depth-map fusion -- next to the other mesh headers: the new header declares exactly three names and two
constants, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the headers of include/, their lists and the
ABI number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import inspect
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "aaai2023-pvd_amd", "csrc")
NAMES = ["pvd_mesh_tsdf_finalize", "pvd_mesh_tsdf_integrate", "pvd_mesh_tsdf_sample_color"]
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


def test_the_header_declares_exactly_the_three_names_and_the_constants():
    path = os.path.join(CSRC, "pvd_hip_mesh_tsdf.h")
    assert _declared(path) == NAMES
    src = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert dict(re.findall(r"^#define (PVD_MESH_TSDF_[A-Z_]+) (\S+)$", code, flags=re.M)) == {"PVD_MESH_TSDF_MAX_R": "1024",
                                                                                             "PVD_MESH_TSDF_MAX_SIDE": "16384"}
    assert '#include "../../include/pvd_hip.h"' in code
    # the definition is in the header, operation by operation
    assert "NOTHING IS FUSED" in src
    for line in ("c_a(n) = (float)n / (float)(R - 1) * (hi_a - lo_a) + lo_a",
                 "d   = p - o",
                 "q_a = (M[0][a] * d_x + M[1][a] * d_y) + M[2][a] * d_z",
                 "q_z > 0, or the view is skipped",
                 "x = (fx * q_x) / q_z + cx,      y = (fy * q_y) / q_z + cy",
                 "0 <= x < W and 0 <= y < H, or the view is skipped",
                 "i = (int)floorf(x),  j = (int)floorf(y)",
                 "D = depth[v][j][i];  D > 0, or the view is skipped",
                 "r = sqrtf((d_x * d_x + d_y * d_y) + d_z * d_z)",
                 "s = D - r",
                 "s >= -tau, or the view is skipped",
                 "t = fminf(s / tau, 1)",
                 "w = weight[v][j][i], or 1;  0 < w < +inf, or the view is skipped",
                 "acc_d = acc_d + w * t",
                 "acc_w = acc_w + w",
                 "acc_c[c] = acc_c[c] + w * color[v][j][i][c]",
                 "acc_w >= min_weight:  field = fmaxf(fminf(acc_d / acc_w, 1), -1)",
                 "u_a = (P_a - lo_a) / (hi_a - lo_a) * r1",
                 "i_a = min((int)floorf(u_a), R - 2)",
                 "m_abc = (h_x * h_y) * h_z",
                 "M = M + m_abc;        C_c = C_c + m_abc * (acc_c[c] / acc_w)",
                 "M > 0:  colors[c] = fminf(fmaxf(C_c / M, 0), 1)"):
        assert line in src, line
    assert "unknown = -1 treats unseen space as solid" in src and "unknown = +1 treats unseen space as empty" in src
    assert "in ascending order" in src and "views can arrive in batches" in src and "not staged in LDS and not chunked" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared(_include("pvd_hip.h"))) == 75
    assert set(OTHERS) == set(os.listdir(os.path.join(REPO, "include")))
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(_include(h))), h
        assert "PVD_MESH_TSDF_" not in open(_include(h)).read(), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_TSDF, tuple) and sorted(pvd_hip.ENTRY_POINTS_MESH_TSDF) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(_include(header)), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_TSDF) & set(getattr(pvd_hip, tup)), header
    assert not set(pvd_hip.ENTRY_POINTS_MESH_TSDF) & (set(pvd_hip.ENTRY_POINTS_MESH_EXPOSE) | set(pvd_hip.ENTRY_POINTS_MESH_SHTEX))
    for name in NAMES:
        assert callable(getattr(pvd_hip, name[len("pvd_"):]))
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_TSDF_MAX_R == 1024 and pvd_hip.MESH_TSDF_MAX_SIDE == 16384
    assert pvd_hip.MESH_TSDF_TOTALS == ("observed", "observed_inside", "unknown")
    import mesh_tsdf_restatement as tr
    assert tr.MAX_R == 1024 and tr.MAX_SIDE == 16384


def test_the_source_and_the_header_are_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert "mesh_tsdf.hip" in srcs and " pvd_hip_mesh_tsdf.h " in mk
    assert "-ffp-contract=off" in [ln for ln in mk.splitlines() if ln.startswith("FLAGS")][0]
    src = open(os.path.join(CSRC, "mesh_tsdf.hip")).read()
    assert '#include "pvd_hip_mesh_tsdf.h"' in src and "#pragma clang fp contract(off)" in src
    assert "fma(" not in src and "fmaf(" not in src and "__shared__" not in src
    kernel = src[src.index("void k_tsdf_integrate"):src.index("void k_tsdf_finalize")]
    assert "atomic" not in kernel  # the integration: no atomics; the totals of the finalize pass are integer atomics per wave
    assert "atomicAdd(&totals" in src and "__ballot" in src


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """Unsupported sizes first (R outside 2 .. 1024, H or W outside 1 .. 16384): PVD_ERR_UNSUPPORTED; then a tau or a min_weight that
    is not positive and finite: PVD_ERR_INVALID; then nothing to do (V or N of 0): PVD_OK with no launch, NULL pointers allowed; then
    NULL pointers: PVD_ERR_INVALID -- all before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p
    one, null = vp(64), vp(0)
    for name in NAMES:
        getattr(lib, name).restype = ctypes.c_int
    inf, nan = float("inf"), float("nan")

    def integrate(depth=one, color=one, weight=one, poses=one, intr=one, V=3, H=5, W=7, R=9, lo=one, hi=one, tau=0.1, acc_d=one,
                  acc_w=one, acc_c=one):
        return lib.pvd_mesh_tsdf_integrate(depth, color, weight, poses, intr, u32(V), u32(H), u32(W), u32(R), lo, hi, f32(tau), acc_d, acc_w,
                                           acc_c, null)
    assert integrate(R=1) == -2 and integrate(R=0) == -2 and integrate(R=1025) == -2 and integrate(R=1, V=0) == -2
    assert integrate(H=0) == -2 and integrate(W=0) == -2 and integrate(H=16385) == -2 and integrate(W=16385) == -2
    for bad in (0.0, -1.0, inf, nan):
        assert integrate(tau=bad) == -1 and integrate(tau=bad, V=0) == -1, bad
    assert integrate(V=0) == 0
    assert integrate(V=0, depth=null, color=null, weight=null, poses=null, intr=null, lo=null, hi=null, acc_d=null, acc_w=null, acc_c=null) == 0
    for k in ("depth", "poses", "intr", "lo", "hi", "acc_d", "acc_w"):
        assert integrate(**{k: null}) == -1, k

    def finalize(acc_d=one, acc_w=one, R=9, min_weight=1.0, unknown=-1.0, field=one, totals=one):
        return lib.pvd_mesh_tsdf_finalize(acc_d, acc_w, u32(R), f32(min_weight), f32(unknown), field, totals, null)
    assert finalize(R=1) == -2 and finalize(R=1025) == -2 and finalize(R=1, acc_d=null) == -2
    for bad in (0.0, -1.0, inf, nan):
        assert finalize(min_weight=bad) == -1, bad
    assert finalize(unknown=inf) == -1 and finalize(unknown=nan) == -1
    for k in ("acc_d", "acc_w", "field", "totals"):
        assert finalize(**{k: null}) == -1, k

    def sample(acc_c=one, acc_w=one, R=9, lo=one, hi=one, min_weight=1.0, points=one, N=5, colors=one):
        return lib.pvd_mesh_tsdf_sample_color(acc_c, acc_w, u32(R), lo, hi, f32(min_weight), points, u32(N), colors, null)
    assert sample(R=1) == -2 and sample(R=1025) == -2 and sample(R=1, N=0) == -2
    for bad in (0.0, -1.0, inf, nan):
        assert sample(min_weight=bad) == -1 and sample(min_weight=bad, N=0) == -1, bad
    assert sample(N=0) == 0 and sample(N=0, acc_c=null, acc_w=null, lo=null, hi=null, points=null, colors=null) == 0
    for k in ("acc_c", "acc_w", "lo", "hi", "points", "colors"):
        assert sample(**{k: null}) == -1, k


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import torch
    import pvd_hip
    from pvd import mesh
    z = torch.zeros
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_tsdf_integrate(z(1, 5, 7), None, None, z(1, 4, 4), z(1, 4), 3, z(3), z(3), 0.5, z(27), z(27), None)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_tsdf_finalize(z(27), z(27), 3, 1.0, -1.0, z(27), z(3, dtype=torch.int64))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_tsdf_sample_color(z(27, 3), z(27), 3, z(3), z(3), 1.0, z(4, 3), z(4, 3))
    with pytest.raises(ValueError):
        mesh.tsdf_volume(1, (-1, -1, -1), (1, 1, 1), device="cpu")
    with pytest.raises(ValueError):
        mesh.tsdf_volume(8, (-1, -1, -1), (1, 1, 1), tau=0.0, device="cpu")
    vol = mesh.tsdf_volume(9, (-1, -1, -1), (1, 2, 1), device="cpu")  # the default tau: 3 spacings of the longest axis
    assert vol.R == 9 and abs(vol.tau - 3 * 3.0 / 8) < 1e-6 and tuple(vol.acc_c.shape) == (9, 9, 9, 3) and vol.views == 0
    assert mesh.tsdf_volume(9, (-1, -1, -1), (1, 1, 1), with_color=False, device="cpu").acc_c is None
    with pytest.raises(ValueError):  # a volume with colour refuses a view without: its weight would darken the fused colours
        mesh.tsdf_integrate(vol, z(1, 5, 7), z(1, 4, 4), (7.0, 5.0, 3.5, 2.5))
    assert vol.views == 0 and not vol.acc_w.any()
    poses = mesh.tsdf_poses(16)
    assert tuple(poses.shape) == (16, 4, 4) and torch.allclose(poses[:, :3, 3].norm(dim=1), torch.full((16,), 3.2), atol=1e-5)
    # every default camera looks at the origin along its +z (get_rays' convention)
    assert torch.allclose(poses[:, :3, 2], -poses[:, :3, 3] / 3.2, atol=1e-5)
    # the existing signatures keep their defaults
    sig = inspect.signature(mesh.extract_surface).parameters
    assert sig["texture"].default == 0 and sig["texture_sh"].default == 0 and sig["threshold"].default is None
    sig = inspect.signature(mesh.extract_surface_tsdf).parameters
    assert [sig[k].default for k in ("resolution", "tau", "views_per_batch", "simplify", "texture")] == [256, None, 8, 0, 0]
    sig = inspect.signature(mesh.render_depth_maps).parameters
    assert [sig[k].default for k in ("min_opacity", "free_opacity", "max_steps")] == [0.5, 0.05, 1024]
