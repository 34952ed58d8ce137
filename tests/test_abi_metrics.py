"""include/pvd_hip_metrics.h -- SSIM + squared error of image pairs -- next to include/pvd_hip.h: the new header declares exactly two
names, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and the first header, its list and the ABI number
are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_metrics_header_declares_exactly_the_two_entry_points():
    assert _declared("pvd_hip_metrics.h") == ["pvd_image_metrics", "pvd_image_metrics_workspace_floats"]
    src = _source("pvd_hip_metrics.h")
    assert '#include "pvd_hip.h"' in src
    for cite in ("utils.py:219-300", "utils.py:1275-1279", "utils.py:491-529"):
        assert cite in src, cite


def test_the_library_exports_them_and_the_first_header_is_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for s in _declared("pvd_hip_metrics.h"):
        assert hasattr(lib, s), "libpvd_hip.so does not export %s" % s
    first = set(_declared("pvd_hip.h"))
    assert len(first) == 75 and not first & set(_declared("pvd_hip_metrics.h")) and not set(_declared("pvd_hip_mlp.h")) & set(_declared("pvd_hip_metrics.h"))
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert sorted(pvd_hip.ENTRY_POINTS_METRICS) == _declared("pvd_hip_metrics.h")
    assert sorted(pvd_hip.ENTRY_POINTS) == _declared("pvd_hip.h")
    assert callable(pvd_hip.image_metrics) and callable(pvd_hip.image_metrics_workspace_floats)
    # the constants the binding repeats are the header's
    src = _source("pvd_hip_metrics.h")
    assert pvd_hip.METRICS_TILE == int(re.search(r"#define PVD_METRICS_TILE (\d+)", src).group(1))
    assert pvd_hip.METRICS_MAX_FILTER == int(re.search(r"#define PVD_METRICS_MAX_FILTER (\d+)", src).group(1))


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """B == 0 is PVD_OK, NULL pointers and empty images PVD_ERR_INVALID, an even window, one above 15 taps and C outside 1..4
    PVD_ERR_UNSUPPORTED -- all before a device is touched; the workspace size follows the tile count."""
    lib = ctypes.CDLL(hip_lib_built)
    import pvd_hip
    u32, f32, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p
    one = vp(16)  # a non-NULL value that is never dereferenced on these paths
    taps = (ctypes.c_float * 16)(*([1.0 / 16] * 16))

    def call(B=1, H=8, W=8, C=3, fs=11, img0=one, taps=taps, ws=one, ssim=one):
        return lib.pvd_image_metrics(img0, one, u32(B), u32(H), u32(W), u32(C), taps, u32(fs), f32(0.01), f32(0.03), f32(1.0), ws, ssim, one, vp(0), vp(0))
    assert call(B=0) == 0 and call(B=0, img0=vp(0), fs=4, C=9) == 0
    assert call(img0=vp(0)) == -1 and call(taps=None) == -1 and call(ws=vp(0)) == -1 and call(ssim=vp(0)) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(fs=10) == -2 and call(fs=0) == -2 and call(fs=17) == -2 and call(C=5) == -2 and call(C=0) == -2

    T = pvd_hip.METRICS_TILE
    size = lib.pvd_image_metrics_workspace_floats
    size.restype = ctypes.c_int
    base = size(u32(0), u32(8), u32(8), u32(3))
    assert base > 0
    assert size(u32(1), u32(T), u32(T), u32(3)) == base + 2
    assert size(u32(1), u32(T + 1), u32(T), u32(3)) == base + 4
    assert size(u32(3), u32(2 * T + 1), u32(T + 1), u32(1)) == base + 2 * 3 * 3 * 2
    assert size(u32(4096), u32(1 << 20), u32(1 << 20), u32(3)) == -2  # more tiles than a launch takes
