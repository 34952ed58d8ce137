"""csrc/pvd_hip_mesh_shtex.h -- the view-dependent atlas -- next to the other mesh headers: the new header declares exactly four names
and one constant, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the headers of include/, their lists
and the ABI number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import inspect
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "aaai2023-pvd_amd", "csrc")
NAMES = ["pvd_mesh_shtex_basis", "pvd_mesh_shtex_dirs", "pvd_mesh_shtex_project", "pvd_mesh_shtex_sample"]
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


def test_the_header_declares_exactly_the_four_names_and_the_constant():
    path = os.path.join(CSRC, "pvd_hip_mesh_shtex.h")
    assert _declared(path) == NAMES
    src = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert dict(re.findall(r"^#define (PVD_MESH_SHTEX_[A-Z_]+) (\S+)$", code, flags=re.M)) == {"PVD_MESH_SHTEX_MAX_L": "4"}
    assert '#include "../../include/pvd_hip_mesh_tex.h"' in code
    # the definition is in the header: sixteen polynomials with float32 literals, the mirrored direction, the projection, the sample
    assert "NOTHING IS FUSED" in src and len(re.findall(r"^ \*\s+Y_(\d+)\s+=", src, flags=re.M)) == 16
    assert "Y_9  = -0.590043604f * (y * (3.0f * xx - yy))" in src and "Y_6  =  0.946174681f * zz - 0.31539157f" in src
    assert "r = (2 * s) / q" in src and "d = u - r * n" in src and "acc = acc + P[k][j] * rgb[j][t][c]" in src
    assert "out  = fminf(fmaxf(c, 0), 1)" in src and "(k ascending)" in src


def test_the_restatement_carries_the_header_s_literals():
    """Every float literal of the header's basis appears in the numpy restatement, in the kernel and in pvd/mesh.py's host form."""
    src = open(os.path.join(CSRC, "pvd_hip_mesh_shtex.h")).read()
    block = src[src.index("Y_0  ="):src.index("Each is the real polynomial")]
    literals = sorted(set(re.findall(r"(\d\.\d+)f", block)))
    assert len(literals) == 14, literals  # thirteen constants and 3.0
    kernel = open(os.path.join(CSRC, "mesh_shtex.hip")).read()
    rest = open(os.path.join(HERE, "mesh_shtex_restatement.py")).read()
    host = open(os.path.join(REPO, "aaai2023-pvd_amd", "pvd", "mesh.py")).read()
    for lit in literals:
        assert lit + "f" in kernel and lit + ")" in rest and lit + ")" in host, lit


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for name in NAMES:
        assert hasattr(lib, name), "libpvd_hip.so does not export " + name
    assert len(_declared(_include("pvd_hip.h"))) == 75
    assert _declared(_include("pvd_hip_mesh_tex.h")) == ["pvd_mesh_tex_layout", "pvd_mesh_tex_points", "pvd_mesh_tex_sample"]
    assert set(OTHERS) == set(os.listdir(os.path.join(REPO, "include")))
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(_include(h))), h
        assert "PVD_MESH_SHTEX_" not in open(_include(h)).read(), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert isinstance(pvd_hip.ENTRY_POINTS_MESH_SHTEX, tuple) and sorted(pvd_hip.ENTRY_POINTS_MESH_SHTEX) == NAMES
    for header, tup in OTHERS.items():
        assert sorted(getattr(pvd_hip, tup)) == _declared(_include(header)), header
        assert not set(pvd_hip.ENTRY_POINTS_MESH_SHTEX) & set(getattr(pvd_hip, tup)), header
    assert not set(pvd_hip.ENTRY_POINTS_MESH_SHTEX) & set(pvd_hip.ENTRY_POINTS_MESH_EXPOSE)
    for name in NAMES:
        assert callable(getattr(pvd_hip, name[len("pvd_"):]))
    assert pvd_hip.ABI_VERSION == 6 and pvd_hip.MESH_SHTEX_MAX_L == 4
    import mesh_shtex_restatement as sr
    assert sr.MAX_L == 4


def test_the_source_and_the_header_are_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert "mesh_shtex.hip" in srcs and srcs.index("mesh_shtex.hip") == srcs.index("mesh_tex.hip") + 1
    assert " pvd_hip_mesh_shtex.h " in mk and " mesh_atlas.h " in mk
    assert "-ffp-contract=off" in [ln for ln in mk.splitlines() if ln.startswith("FLAGS")][0]
    src = open(os.path.join(CSRC, "mesh_shtex.hip")).read()
    assert '#include "pvd_hip_mesh_shtex.h"' in src and "#pragma clang fp contract(off)" in src
    assert "fma(" not in src and "fmaf(" not in src and "__shared__" not in src and "atomic" not in src.replace("no atomics", "")
    assert "sh_basis.inc" not in src and "pvd_sh_basis" not in src  # the fused basis of the direction encoder is not this one
    assert "void texel_of(" not in src  # the atlas addressing is csrc/mesh_atlas.h's, shared with mesh_tex.hip, not a copy
    for L in "1234":  # the band count is a template parameter with four instantiations
        assert "k_st_sample<%s>" % L in src


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """Unsupported sizes first (the layout's S and side, L outside 1 .. 4): PVD_ERR_UNSUPPORTED; then nothing to do (N, M or J of 0):
    PVD_OK with no launch, NULL pointers allowed; then NULL pointers: PVD_ERR_INVALID -- all before a device is touched (the pointers
    are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    one, null = vp(64), vp(0)
    for name in NAMES:
        getattr(lib, name).restype = ctypes.c_int

    def basis(dirs=one, N=5, L=3, out=one):
        return lib.pvd_mesh_shtex_basis(dirs, u32(N), u32(L), out, null)
    assert basis(L=0) == -2 and basis(L=5) == -2 and basis(L=0, N=0) == -2 and basis(L=5, dirs=null) == -2
    assert basis(N=0) == 0 and basis(N=0, dirs=null, out=null) == 0
    assert basis(dirs=null) == -1 and basis(out=null) == -1

    def dirs(n=one, M=5, U=one, J=3, d=one):
        return lib.pvd_mesh_shtex_dirs(n, u32(M), U, u32(J), d, null)
    assert dirs(M=0) == 0 and dirs(J=0) == 0 and dirs(M=0, n=null, U=null, d=null) == 0 and dirs(J=0, n=null, U=null, d=null) == 0
    assert dirs(n=null) == -1 and dirs(U=null) == -1 and dirs(d=null) == -1

    def project(rgb=one, P=one, L=3, J=3, M=5, coef=one, first=1):
        return lib.pvd_mesh_shtex_project(rgb, P, u32(L), u32(J), u32(M), coef, u32(first), null)
    assert project(L=0) == -2 and project(L=5) == -2 and project(L=5, M=0) == -2 and project(L=0, rgb=null) == -2
    assert project(M=0) == 0 and project(J=0) == 0 and project(M=0, rgb=null, P=null, coef=null) == 0
    assert project(J=0, rgb=null, P=null, coef=null, first=0) == 0
    assert project(rgb=null) == -1 and project(P=null) == -1 and project(coef=null) == -1

    def sample(tex=one, T=5, S=8, L=3, tri=one, bary=one, d=one, N=7, bg=one, color=one):
        return lib.pvd_mesh_shtex_sample(tex, u32(T), u32(S), u32(L), tri, bary, d, u32(N), bg, color, null)
    assert sample(S=3) == -2 and sample(S=65) == -2 and sample(T=2 ** 31, S=64) == -2  # the layout's errors
    assert sample(L=0) == -2 and sample(L=5) == -2
    assert sample(S=3, N=0) == -2 and sample(L=5, N=0) == -2 and sample(L=0, tex=null) == -2  # the limits first
    assert sample(N=0) == 0 and sample(N=0, tex=null, tri=null, bary=null, d=null, bg=null, color=null) == 0
    assert sample(T=0, N=0) == 0
    for k in ("tex", "tri", "bary", "d", "bg", "color"):
        assert sample(**{k: null}) == -1, k


def test_the_binding_rejects_cpu_tensors_and_wrong_shapes(hip_lib_built):
    import torch
    import pvd_hip
    from pvd import mesh
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_shtex_basis(torch.ones(4, 3), 2, torch.zeros(4, 4))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_shtex_dirs(torch.ones(4, 3), torch.ones(2, 3), torch.zeros(2, 4, 3))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_shtex_project(torch.ones(2, 4, 3), torch.ones(4, 2), 2, torch.zeros(4, 4, 3), True)
    with pytest.raises(pvd_hip.PvdHipError):
        mesh.sample_sh_texture(torch.zeros(8, 8, 4, 3), 8, 2, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2), torch.ones(1, 3))
    with pytest.raises(ValueError):
        mesh.sample_sh_texture(torch.zeros(8, 8, 5, 3), 8, 2, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2), torch.ones(1, 3))
    with pytest.raises(ValueError):
        mesh.sh_basis(torch.ones(2, 3), 5)
    # the existing signatures keep their defaults; the new arguments are off by default
    sig = inspect.signature(mesh.extract_surface).parameters
    assert sig["texture"].default == 0 and sig["texture_sh"].default == 0
    sig = inspect.signature(mesh.bake_sh_texture).parameters
    assert [sig[k].default for k in ("degree", "dirs", "normals", "chunk", "batch")] == [3, None, None, 1 << 20, 8]
    assert inspect.signature(mesh.sample_sh_texture).parameters["bg_color"].default == 1.0
    assert inspect.signature(mesh.render_mesh).parameters["texture"].default is None
