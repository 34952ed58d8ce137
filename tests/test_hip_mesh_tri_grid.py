"""The triangle grid of csrc/mesh_tri_grid.h as pvd_mesh_ray_build (three binned axes) and pvd_mesh_winding_build (two) leave it in
their workspace, against tests/mesh_tri_grid_restatement.py: exactly, up to the order of the pairs inside a cell and of the outside
list.  The workspace is decoded by the byte formula of the public headers,
    64 + 48 T + 4 (C + 1) + 4 C + 4 ceil(C / 256) + 4 T + 4 pairs,        C = G^3 or G^2:
the header, the packed records, the starts, the cursors, the partial sums, the outside list, the pairs.

Sizes.  The mesh is the ("sphere", 9) fixture (648 triangles: three workgroups of the per-triangle passes, the last one partial), its
first 257 triangles (one lane into a second workgroup), the same mesh with four invalid triangles, and no triangles at all (the box
must still reach the header).  G = 1 (one cell), 2 and 7 (343 or 49 cells: a partial workgroup of the per-cell passes, and for three
axes a second one).  The boxes: the mesh's own (nothing outside, triangles that touch bmax), one much smaller than the mesh (most
triangles outside: all of this mesh's) and one with a flat axis and an axis of negative extent; and, so that one build has both
lists, the half x <= 0 of the fixtures' box.

No case reaches a second chunk of the scan of the per-workgroup sums: test_the_scan_of_the_cell_counts_carries_into_a_second_chunk of
tests/test_hip_mesh_ray.py covers it at G = 129 for three axes, and two axes cannot reach it -- 1024^2 / 256 = 4096 sums at the
largest G are below the 8192 of one chunk."""
import functools

import numpy as np
import pytest
import torch

import mesh_dist_restatement as md
import mesh_tri_grid_restatement as tg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
APIS = {"mesh_ray": 3, "mesh_winding": 2}  # the binding's prefix -> the binned axes
GS = (1, 2, 7)
BOXES = {"own": None,  # the bounding box of the fixture's vertices
         "small": ((0.1, 0.6, 1.0), (0.2, 0.7, 1.1)),  # much smaller than the mesh (tests/test_hip_mesh_ray.py)
         "flat": ((-1.0, -0.5, 0.25), (1.0, -0.5, 0.0)),  # one flat axis and one of negative extent (tests/test_hip_mesh_ray.py)
         "half": ((-1.0, -1.0, -1.0), (0.0, 1.0, 1.0))}  # cuts the mesh: inside and outside triangles in one build
MESHES = ("whole", "first_257", "four_invalid", "none")


@functools.lru_cache(maxsize=None)
def _mesh(which):
    v, t = md.fixture("sphere", 9)
    if which == "first_257":
        t = t[:257]
    elif which == "none":
        t = t[:0]
    elif which == "four_invalid":
        V = len(v) + 2
        v = np.concatenate([v, np.array([(np.nan, 0.0, 0.1), (0.0, np.inf, 0.1)], np.float32)])
        t = t.copy()
        t[5, 2], t[100, 1], t[300, 0], t[301, 1] = V, -1, V - 2, V - 1  # an index equal to V, a negative one, a NaN and an infinite corner
        assert md.valid_triangles(v, t).sum() == len(t) - 4
    return np.array(v), np.array(t)  # writable copies: the fixture is read-only


def _box(name):
    if BOXES[name] is not None:
        return BOXES[name]
    v = md.fixture("sphere", 9)[0]
    return tuple(v.min(axis=0).tolist()), tuple(v.max(axis=0).tolist())


def _decode(ws, T, C, pairs):
    """The sections of the workspace, in the order of the headers' formula."""
    sizes = (("header", 64), ("records", 48 * T), ("start", 4 * (C + 1)), ("cursor", 4 * C), ("bsum", 4 * -(-C // 256)), ("outside", 4 * T),
             ("pairs", 4 * pairs))
    assert len(ws) == sum(n for _, n in sizes)
    out, at = {}, 0
    for name, n in sizes:
        out[name] = np.frombuffer(ws[at:at + n].tobytes(), np.uint32)
        at += n
    return out


@pytest.mark.parametrize("box", sorted(BOXES))
@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("api", sorted(APIS))
def test_count_and_build_leave_the_restatements_grid(api, mesh, box):
    import pvd_hip
    axes = APIS[api]
    count, nbytes, build = (getattr(pvd_hip, "%s_%s" % (api, f)) for f in ("count", "workspace_bytes", "build"))
    v, t = _mesh(mesh)
    T = len(t)
    bmin, bmax = _box(box)
    vt, tt = torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV)
    lo, hi = torch.tensor(bmin, dtype=torch.float32, device=DEV), torch.tensor(bmax, dtype=torch.float32, device=DEV)
    for G in GS:
        label = "%s %s %s G=%d" % (api, mesh, box, G)
        ref = tg.grid(v, t, bmin, bmax, G, axes)
        C = G ** axes
        totals = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        count(vt, tt, lo, hi, G, totals)
        print(label, "totals", totals.tolist(), "restatement", (ref["pairs"], ref["n_outside"]))
        assert totals.tolist() == [ref["pairs"], ref["n_outside"]], label
        pairs = ref["pairs"]
        ws = torch.full((nbytes(T, G, pairs),), 0xAB, dtype=torch.uint8, device=DEV)
        build(vt, tt, lo, hi, G, pairs, ws)
        w = _decode(ws.cpu().numpy(), T, C, pairs)
        header, start = w["header"], w["start"]
        assert header[0] == ref["n_outside"] and header[7] == pairs and start[C] == pairs, label
        assert header[1:7].tobytes() == np.array(bmin + bmax, np.float32).tobytes(), label
        sizes = np.array([len(c) for c in ref["cells"]], np.int64)
        assert np.array_equal(start[:C], np.cumsum(sizes) - sizes), label  # the exclusive prefix sum
        assert np.array_equal(w["cursor"], start[1:]), label  # every cell was filled to the next cell's start
        for c in range(C):
            assert sorted(w["pairs"][start[c]:start[c + 1]].tolist()) == ref["cells"][c], (label, c)
        assert np.array_equal(np.sort(w["outside"][:ref["n_outside"]]), ref["outside"]), label
        assert w["records"].tobytes() == ref["records"].tobytes(), label
