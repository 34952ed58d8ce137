"""include/pvd_hip_mlp.h -- the inference entry points of the frozen `mlp` model -- next to include/pvd_hip.h: the new header declares
exactly two names, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the first header, its list and the
ABI number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _declared(header):
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_mlp_header_declares_exactly_the_two_entry_points():
    assert _declared("pvd_hip_mlp.h") == ["pvd_infer_image_mlp", "pvd_mlp_head_forward_fused_rows"]
    src = open(os.path.join(REPO, "include", "pvd_hip_mlp.h")).read()
    assert '#include "pvd_hip.h"' in src
    for cite in ("network.py:154-182", ":413-437", "renderer.py:450-543"):
        assert cite in src, cite


def test_the_library_exports_them_and_the_first_header_is_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for s in _declared("pvd_hip_mlp.h"):
        assert hasattr(lib, s), "libpvd_hip.so does not export %s" % s
    assert len(_declared("pvd_hip.h")) == 75 and not set(_declared("pvd_hip.h")) & set(_declared("pvd_hip_mlp.h"))
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert sorted(pvd_hip.ENTRY_POINTS_MLP) == _declared("pvd_hip_mlp.h")
    assert sorted(pvd_hip.ENTRY_POINTS) == _declared("pvd_hip.h")
    assert callable(pvd_hip.infer_image_mlp) and callable(pvd_hip.mlp_head_forward_fused)
    import inspect
    assert "rows_dev" in inspect.signature(pvd_hip.mlp_head_forward_fused).parameters


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """Both return through their argument checks without touching a device: N == 0 / M == 0 are PVD_OK, NULL pointers PVD_ERR_INVALID,
    a positional encoding other than 10 bands PVD_ERR_UNSUPPORTED (no GPU is needed for these paths)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p
    one = vp(16)  # a non-NULL value that is never dereferenced on these paths
    bands = (ctypes.c_float * 10)(*[2.0 ** k for k in range(10)])

    def infer(N=4, rays_o=one, n_freqs=10, bands=bands, wstream=one, n_before=3, max_steps=1024):
        return lib.pvd_infer_image_mlp(rays_o, one, one, one, u32(N), one, f32(1.0), f32(0.0), u32(max_steps), u32(1), u32(128), f32(1.0), bands,
                                       u32(n_freqs), wstream, u32(n_before), u32(2), one, one, one, one, one, vp(0), f32(-2.0), f32(7.0), one, one,
                                       one, one, vp(0))
    assert infer(N=0) == 0
    assert infer(rays_o=vp(0)) == -1 and infer(wstream=vp(0)) == -1 and infer(bands=None) == -1 and infer(max_steps=0) == -1
    assert infer(n_freqs=6) == -2 and infer(n_before=17) == -2

    def rows(M=4, pts=one, n_before=3):
        return lib.pvd_mlp_head_forward_fused_rows(pts, u32(M), one, u32(n_before), u32(2), one, one, one, one, one, one, vp(0), f32(-2.0), f32(7.0),
                                                   one, one, one, one, vp(0))
    assert rows(M=0) == 0 and rows(pts=vp(0)) == -1 and rows(n_before=17) == -2
