"""include/pvd_hip_data.h -- training batches drawn on the device from a uint8 image stack, and the error-map feedback -- next to
include/pvd_hip.h: the new header declares exactly two names, libpvd_hip.so exports them, the binding lists them in a tuple of their
own, and the first header, its list and the ABI number are what they were (no compute calls: this runs without a GPU; hipcc
cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OTHER_HEADERS = ("pvd_hip.h", "pvd_hip_mlp.h", "pvd_hip_metrics.h")


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_data_header_declares_exactly_the_two_entry_points():
    assert _declared("pvd_hip_data.h") == ["pvd_error_map_update", "pvd_image_batch"]
    src = _source("pvd_hip_data.h")
    assert '#include "pvd_hip.h"' in src
    for cite in ("provider.py:278-308", "utils.py:324-404", ":357-381", "utils.py:987-995", "utils.py:1120-1129"):
        assert cite in src, cite


def test_the_library_exports_them_and_the_first_header_is_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for s in _declared("pvd_hip_data.h"):
        assert hasattr(lib, s), "libpvd_hip.so does not export %s" % s
    assert len(_declared("pvd_hip.h")) == 75
    for h in OTHER_HEADERS:
        assert not set(_declared(h)) & set(_declared("pvd_hip_data.h")), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert sorted(pvd_hip.ENTRY_POINTS_DATA) == _declared("pvd_hip_data.h")
    assert sorted(pvd_hip.ENTRY_POINTS) == _declared("pvd_hip.h") and len(pvd_hip.ENTRY_POINTS) == 75
    assert sorted(pvd_hip.ENTRY_POINTS_METRICS) == _declared("pvd_hip_metrics.h")
    assert callable(pvd_hip.image_batch) and callable(pvd_hip.error_map_update)
    assert pvd_hip.DATA_MAX_GRID == int(re.search(r"#define PVD_DATA_MAX_GRID (\d+)", _source("pvd_hip_data.h")).group(1)) == 128


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """N == 0 is PVD_OK whatever else is passed; NULL required pointers, H W >= 2^32, C outside {3, 4}, RGBA without bg and, with an
    error map, N > g*g or no inds_coarse are PVD_ERR_INVALID; g == 0 and g > 128 with an error map PVD_ERR_UNSUPPORTED -- all before
    a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, u64, f32, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p
    one, null = vp(16), vp(0)  # `one`: a non-NULL value that is never dereferenced on these paths
    names = ("images", "poses", "order", "state", "aabb", "error_map", "view_out", "inds", "inds_coarse", "rays_o", "rays_d", "gt", "bg",
             "nears", "fars", "keys_out")

    def batch(V=3, H=20, W=28, C=4, N=100, g=8, **ptr):
        p = {n: one for n in names}
        p.update(error_map=null, keys_out=null)
        p.update(ptr)
        return lib.pvd_image_batch(p["images"], p["poses"], p["order"], u32(V), u32(H), u32(W), u32(C), p["state"], u64(7), f32(30.0), f32(30.0),
                                   f32(14.0), f32(10.0), u32(N), p["aabb"], f32(0.2), p["error_map"], u32(g), p["view_out"], p["inds"],
                                   p["inds_coarse"], p["rays_o"], p["rays_d"], p["gt"], p["bg"], p["nears"], p["fars"], p["keys_out"], null)
    assert batch(N=0) == 0 and batch(N=0, images=null, C=9, g=0, error_map=one) == 0
    for required in ("images", "poses", "state", "aabb", "view_out", "inds", "rays_o", "rays_d", "gt", "nears", "fars"):
        assert batch(**{required: null}) == -1, required
    assert batch(V=0) == -1 and batch(H=0) == -1 and batch(W=0) == -1
    assert batch(H=1 << 16, W=1 << 16) == -1 and batch(H=1 << 20, W=1 << 20) == -1
    assert batch(C=0) == -1 and batch(C=1) == -1 and batch(C=2) == -1 and batch(C=5) == -1
    assert batch(C=4, bg=null) == -1
    assert batch(error_map=one, g=8, N=65) == -1 and batch(error_map=one, g=128, N=128 * 128 + 1) == -1
    assert batch(error_map=one, inds_coarse=null) == -1
    assert batch(error_map=one, g=0) == -2 and batch(error_map=one, g=129) == -2 and batch(error_map=one, g=1 << 16, N=1) == -2

    def update(g=8, N=10, **ptr):
        p = {n: one for n in ("error_map", "view", "inds_coarse", "pred", "gt")}
        p.update(ptr)
        return lib.pvd_error_map_update(p["error_map"], u32(g), p["view"], p["inds_coarse"], p["pred"], p["gt"], u32(N), null)
    assert update(N=0) == 0 and update(N=0, error_map=null, g=0) == 0
    for required in ("error_map", "view", "inds_coarse", "pred", "gt"):
        assert update(**{required: null}) == -1, required
    assert update(g=0) == -1
