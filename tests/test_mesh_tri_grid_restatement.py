"""tests/mesh_tri_grid_restatement.py on hand-made cases whose answer can be written down (CPU).  tests/test_hip_mesh_tri_grid.py
compares the device's workspace with the same restatement."""
import numpy as np

import mesh_ray_restatement as rr
import mesh_tri_grid_restatement as tg

EPS = 2.0 ** -20  # of a box of extent 1


def _one(corners, bmin, bmax, G, axes):
    """The grid of the single triangle `corners`."""
    return tg.grid(np.array(corners, np.float32), np.array([(0, 1, 2)], np.int32), bmin, bmax, G, axes)


def _cells_of(g):
    return [i for i, c in enumerate(g["cells"]) if c]


def test_the_unit_cube_in_one_cell():
    for axes in (3, 2):
        g = tg.grid(rr.CUBE_V, rr.CUBE_T, (0, 0, 0), (1, 1, 1), 1, axes)
        assert g["cells"] == [list(range(12))] and g["pairs"] == 12 and g["n_outside"] == 0 and len(g["outside"]) == 0


def test_the_unit_cube_in_two_cells_per_axis():
    """Every triangle spans its face: along the face's normal it lies on the box's wall and stays in the layer next to it (0 - eps
    and 0 + eps are in layer 0; 1 - eps and 1 + eps, clamped, in layer 1), along the other axes it reaches both layers.  The faces:
    z = 0 / 1: triangles 0, 1 / 2, 3; y: 4, 5 / 6, 7; x: 8, 9 / 10, 11."""
    g = tg.grid(rr.CUBE_V, rr.CUBE_T, (0, 0, 0), (1, 1, 1), 2, 3)
    assert g["pairs"] == 12 * 4 and g["n_outside"] == 0
    for x in range(2):
        for y in range(2):
            for z in range(2):
                assert g["cells"][(x * 2 + y) * 2 + z] == sorted([2 * z, 2 * z + 1, 4 + 2 * y, 5 + 2 * y, 8 + 2 * x, 9 + 2 * x]), (x, y, z)
    g = tg.grid(rr.CUBE_V, rr.CUBE_T, (0, 0, 0), (1, 1, 1), 2, 2)  # x and y only: the z faces reach all four cells
    assert g["pairs"] == 4 * 4 + 8 * 2 and g["n_outside"] == 0
    for x in range(2):
        for y in range(2):
            assert g["cells"][x * 2 + y] == sorted([0, 1, 2, 3, 4 + 2 * y, 5 + 2 * y, 8 + 2 * x, 9 + 2 * x]), (x, y)


def test_the_records_of_the_cube():
    """Nine coordinates in input order, the index, the edge directions for two axes (bit 0: b < c, bit 1: c < a, bit 2: a < b), 0."""
    for axes in (3, 2):
        r = tg.grid(rr.CUBE_V, rr.CUBE_T, (0, 0, 0), (1, 1, 1), 2, axes)["records"]
        assert r.dtype == np.uint32 and r.shape == (12, 12)
        assert np.array_equal(r[:, :9].view(np.float32), rr.CUBE_V[rr.CUBE_T].reshape(12, 9))
        assert np.array_equal(r[:, 9], np.arange(12)) and not r[:, 11].any()
        # (0, 2, 3): b < c and a < b; (0, 3, 1): a < b only; (1, 7, 5): a < b only; (4, 7, 6): a < b only
        want = {0: 5, 1: 4, 3: 4, 11: 4}
        for t, bits in want.items():
            assert r[t, 10] == (bits if axes == 2 else 0), (axes, t)


def test_a_triangle_on_a_cell_boundary_is_in_both_cells():
    """x = 0.5 is the face between the layers 0 and 1 of G = 2 over 0 .. 1: (0.5 - eps) * 2 is below 1, (0.5 + eps) * 2 is not."""
    tri = [(0.5, 0.1, 0.1), (0.5, 0.2, 0.1), (0.5, 0.1, 0.2)]
    assert _cells_of(_one(tri, (0, 0, 0), (1, 1, 1), 2, 3)) == [0, 4]  # (0,0,0) and (1,0,0)
    assert _cells_of(_one(tri, (0, 0, 0), (1, 1, 1), 2, 2)) == [0, 2]  # (0,0) and (1,0)
    # one dilation inside the lower cell it stays there, and at G = 4 the same plane is the face between the layers 1 and 2
    inner = [(0.5 - 2 * EPS, y, z) for _, y, z in tri]
    assert _cells_of(_one(inner, (0, 0, 0), (1, 1, 1), 2, 3)) == [0]
    assert _cells_of(_one(tri, (0, 0, 0), (1, 1, 1), 4, 3)) == [16, 32]


def test_a_flat_axis_and_an_axis_of_negative_extent():
    """y has extent 0 and z a negative one: both are flat, one layer from -inf to +inf, and take no part in the inside test; x alone is
    binned (-1 .. 1, four layers of 0.5)."""
    bmin, bmax = (-1.0, -0.5, 0.25), (1.0, -0.5, 0.0)
    flat, lo, hi, inv_h, eps = tg.box_of(bmin, bmax, 4, 3)
    assert flat.tolist() == [False, True, True] and inv_h.tolist() == [2.0, 0.0, 0.0] and eps.tolist() == [2.0 ** -19, 0.0, 0.0]
    tri = [(-0.3, 100.0, -7.0), (0.2, -100.0, 9.0), (0.1, 3.0, 0.1)]  # x from -0.3 to 0.2: layers 1 and 2; far outside in y and z
    g = _one(tri, bmin, bmax, 4, 3)
    assert g["n_outside"] == 0 and _cells_of(g) == [1 * 16, 2 * 16]
    g = _one(tri, bmin, bmax, 4, 2)  # the same on two axes: cell = x * G + 0
    assert g["n_outside"] == 0 and _cells_of(g) == [1 * 4, 2 * 4]
    g = _one([(-1.5, 0, 0), (0, 0, 0), (0, 1, 0)], bmin, bmax, 4, 3)  # past bmin in x: outside
    assert g["n_outside"] == 1 and g["pairs"] == 0
    # a box that is not finite or NaN along an axis is flat there too
    assert tg.box_of((0, 0, 0), (np.inf, np.nan, 1), 2, 3)[0].tolist() == [True, True, False]


def test_touching_bmax_is_inside_and_one_step_past_it_is_outside():
    one, past = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    g = _one([(0.9, 0.9, 0.9), (one, 0.9, 0.9), (0.9, one, one)], (0, 0, 0), (1, 1, 1), 2, 3)
    assert g["n_outside"] == 0 and _cells_of(g) == [7] and g["pairs"] == 1  # 1 + eps is clamped into the last layer
    g = _one([(0.9, 0.9, 0.9), (past, 0.9, 0.9), (0.9, one, one)], (0, 0, 0), (1, 1, 1), 2, 3)
    assert g["n_outside"] == 1 and g["outside"].tolist() == [0] and g["pairs"] == 0 and _cells_of(g) == []
    # z is not a binned axis of the two-axis grid: past the box in z alone is still inside
    g = _one([(0.9, 0.9, 0.9), (one, 0.9, 0.9), (0.9, one, past)], (0, 0, 0), (1, 1, 1), 2, 2)
    assert g["n_outside"] == 0 and _cells_of(g) == [3]


def test_invalid_triangles_are_in_no_list():
    """An index out of range: the record's coordinates are zeros and it has no edge directions; a corner that is not finite: the record
    keeps the coordinates and the directions; both carry the index 0xffffffff."""
    v = np.array([(0.1, 0.1, 0.1), (0.2, 0.1, 0.1), (0.1, 0.2, 0.1), (np.nan, 0.3, 0.3), (np.inf, 0.3, 0.3)], np.float32)
    t = np.array([(0, 1, 2), (0, 1, 5), (0, -1, 2), (0, 1, 3), (2, 1, 4)], np.int32)
    for axes in (3, 2):
        g = tg.grid(v, t, (0, 0, 0), (1, 1, 1), 2, axes)
        assert g["pairs"] == 1 and g["cells"][0] == [0] and g["n_outside"] == 0
        r = g["records"]
        assert r[:, 9].tolist() == [0] + [0xFFFFFFFF] * 4
        assert not r[1:3, :9].any() and not r[1:3, 10].any()
        assert r[3, :9].tobytes() == v[t[3]].tobytes() and r[4, :9].tobytes() == v[t[4]].tobytes()
        assert r[:, 10].tolist() == ([5, 0, 0, 5, 1] if axes == 2 else [0] * 5)  # (2, 1, 4): b < c only


def test_no_triangles():
    g = tg.grid(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), (0, 0, 0), (1, 1, 1), 2, 3)
    assert g["pairs"] == 0 and g["n_outside"] == 0 and g["records"].shape == (0, 12) and g["cells"] == [[]] * 8
