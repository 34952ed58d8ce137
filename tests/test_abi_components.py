"""include/pvd_hip_components.h -- connected components of a density volume's inside set -- next to the other headers: it declares
exactly three names, libpvd_hip.so exports them, the binding lists them in a tuple of their own, and every other header, list and
the ABI number are what they were (no compute calls: this runs without a GPU; hipcc cross-compiles gfx950 on CPU)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = "pvd_hip_components.h"
OTHERS = ("pvd_hip.h", "pvd_hip_mlp.h", "pvd_hip_metrics.h", "pvd_hip_data.h", "pvd_hip_march.h", "pvd_hip_mesh.h")
NAMES = ["pvd_components_filter", "pvd_components_label", "pvd_components_neighbours"]
SLOTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]  # pvd_hip_mesh.h: the owned edges


def _source(header):
    return open(os.path.join(REPO, "include", header)).read()


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", _source(header), flags=re.S)
    return sorted(set(re.findall(r"\b(pvd_[a-zA-Z0-9_]+)\s*\(", src)))


def test_the_header_declares_exactly_the_three_entry_points():
    assert _declared(HEADER) == NAMES
    src = _source(HEADER)
    assert '#include "pvd_hip_mesh.h"' in src
    assert "network.py:601" in src and "utils.py:442-488" in src


def test_the_library_exports_them_and_the_other_headers_are_unchanged(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    for s in NAMES:
        assert hasattr(lib, s), "libpvd_hip.so does not export %s" % s
    assert len(_declared("pvd_hip.h")) == 75
    assert _declared("pvd_hip_mesh.h") == ["pvd_mesh_count", "pvd_mesh_emit", "pvd_mesh_workspace_bytes"]
    for h in OTHERS:
        assert not set(NAMES) & set(_declared(h)), h
    lib.pvd_abi_version.restype = ctypes.c_int
    assert lib.pvd_abi_version() == 6


def test_the_binding_lists_them_in_a_tuple_of_their_own(hip_lib_built):
    import pvd_hip
    assert sorted(pvd_hip.ENTRY_POINTS_COMPONENTS) == NAMES
    assert sorted(pvd_hip.ENTRY_POINTS) == _declared("pvd_hip.h") and len(pvd_hip.ENTRY_POINTS) == 75
    for tup, header in ((pvd_hip.ENTRY_POINTS_MLP, "pvd_hip_mlp.h"), (pvd_hip.ENTRY_POINTS_METRICS, "pvd_hip_metrics.h"),
                        (pvd_hip.ENTRY_POINTS_DATA, "pvd_hip_data.h"), (pvd_hip.ENTRY_POINTS_MARCH, "pvd_hip_march.h"),
                        (pvd_hip.ENTRY_POINTS_MESH, "pvd_hip_mesh.h")):
        assert sorted(tup) == _declared(header), header
        assert not set(NAMES) & set(tup), header
    assert not set(NAMES) & set(pvd_hip.ENTRY_POINTS)
    assert callable(pvd_hip.components_label) and callable(pvd_hip.components_filter) and callable(pvd_hip.components_neighbours)


def test_the_binding_rejects_cpu_tensors(hip_lib_built):
    import pytest
    import torch
    import pvd_hip
    R = 4
    field = torch.zeros(R, R, R)
    labels, sizes = torch.zeros(R ** 3, dtype=torch.int32), torch.zeros(R ** 3, dtype=torch.int32)
    stats, kept = torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.components_label(field, R, 0.0, labels, sizes, stats)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.components_filter(field, labels, sizes, stats, R, 0.0, 1, False, torch.zeros(R, R, R), kept)
    from pvd.mesh import drop_components, label_components
    with pytest.raises(pvd_hip.PvdHipError):
        label_components(field, 0.0)
    with pytest.raises(pvd_hip.PvdHipError):
        drop_components(field, 0.0, min_points=2)


def test_the_entry_points_check_their_arguments_before_any_launch(hip_lib_built):
    """A NULL pointer (or a stats pointer off an 8-byte boundary): PVD_ERR_INVALID; R outside 2..512: PVD_ERR_UNSUPPORTED -- all
    before a device is touched (the pointers are never dereferenced)."""
    lib = ctypes.CDLL(hip_lib_built)
    u32, f32, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p
    one = vp(16)  # a non-NULL value that is never dereferenced on these paths
    lib.pvd_components_label.restype = lib.pvd_components_filter.restype = lib.pvd_components_neighbours.restype = ctypes.c_int

    def label(field=one, R=8, labels=one, sizes=one, stats=one):
        return lib.pvd_components_label(field, u32(R), f32(0.5), labels, sizes, stats, vp(0))

    def filt(field=one, labels=one, sizes=one, stats=one, R=8, out=one, kept=one):
        return lib.pvd_components_filter(field, labels, sizes, stats, u32(R), f32(0.5), u32(3), u32(0), out, kept, vp(0))
    assert label(field=vp(0)) == -1 and label(labels=vp(0)) == -1 and label(sizes=vp(0)) == -1 and label(stats=vp(0)) == -1
    assert label(stats=vp(20)) == -1  # the largest component is found by one 64-bit atomic maximum on stats[2:4]
    assert label(R=0) == -2 and label(R=1) == -2 and label(R=513) == -2 and label(R=2 ** 32 - 1) == -2
    assert label(field=vp(0), R=513) == -1  # the pointers first, as pvd_mesh_count does
    for name in ("field", "labels", "sizes", "stats", "out", "kept"):
        assert filt(**{name: vp(0)}) == -1, name
    assert filt(R=0) == -2 and filt(R=1) == -2 and filt(R=513) == -2
    assert lib.pvd_components_neighbours(vp(0)) == -1


def test_the_neighbours_are_the_meshers_seven_directions_and_their_negatives(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    lib.pvd_components_neighbours.restype = ctypes.c_int
    buf = (ctypes.c_int32 * 44)(*([77] * 44))
    assert lib.pvd_components_neighbours(buf) == 14
    got = [tuple(buf[3 * q:3 * q + 3]) for q in range(14)]
    assert got[:7] == SLOTS and got[7:] == [tuple(-c for c in d) for d in SLOTS] and len(set(got)) == 14
    assert buf[42] == 77 and buf[43] == 77
    mesh = _source("pvd_hip_mesh.h")
    assert "d = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1),\n *          (1,1,1) (edge slots 0..6)" in mesh
    import pvd_hip
    assert pvd_hip.components_neighbours() == got
    import components_restatement as cr
    assert list(cr.OFFSETS) == got
