"""tests/mesh_nets_restatement.py -- the numpy restatement of csrc/pvd_hip_mesh_nets.h -- pinned on its own, without the kernels: hand
cases, the counting identities, the vertex inside its cell, the sequence and split rules, topology on fields with no ambiguous face and
no split cell, derived accuracy bounds on the sphere, and agreement with marching tetrahedra (tests/mesh_restatement.py) within one
cell diagonal.

Measured on this restatement (float32), sphere u = 0.6 - |x| on [-1,1]^3 (profiles/mesh_nets_checks.txt has the table):
    R = 17: |v| - 0.6 in [-8.23e-3, -1.43e-3] against the derived [-1.50e-2, +5.11e-3]; normals within 5.9e-3 (bound 7.8e-1)
    R = 33: [-2.27e-3, -3.65e-4] against [-3.45e-3, +1.00e-3]; normals within 1.5e-3 (bound 7.9e-2)
    R = 65: [-5.84e-4, -9.70e-6] against [-8.39e-4, +2.28e-4]; normals within 4.2e-4 (bound 1.5e-2)
Ambiguous faces and split cells are 0 for the sphere, the shifted sphere and the torus at every R in 5, 9, 17, 33, 65, and the torus has
Euler number 0 from R = 5 on."""
import numpy as np
import pytest

import mesh_nets_restatement as sn
import mesh_restatement as mr

BOX = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
SIZES = (5, 9, 17, 33, 65)
SMOOTH = ("sphere", "shifted", "torus")


@pytest.fixture(scope="module")
def meshes():
    """Computed once, shared, never changed."""
    out = {}
    for kind in SMOOTH:
        for R in SIZES:
            u = sn.field(kind, R)
            m = sn.extract(u, 0.0, *BOX)
            for a in m.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out[kind, R] = (u, m)
    return out


def test_the_edge_numbering_is_the_headers():
    ends = [sn.edge_ends(e) for e in range(12)]
    assert [e[0] for e in ends] == [0] * 4 + [1] * 4 + [2] * 4
    # x edges: A = o_y * 2 + o_z; y edges: b = z, c = x: A = o_z * 1 + o_x * 4; z edges: b = x, c = y: A = o_x * 4 + o_y * 2
    assert [e[3] for e in ends] == [0, 1, 2, 3, 0, 4, 1, 5, 0, 2, 4, 6]
    assert [e[4] - e[3] for e in ends] == [4] * 4 + [2] * 4 + [1] * 4


def test_one_inside_corner_at_R_2_is_one_vertex_at_the_mean_of_three_crossings():
    u = np.full((2, 2, 2), -1.0, np.float32)
    u[0, 0, 0] = 3.0  # t = (0 - 3) / (-1 - 3) = 0.75 on the three edges out of the corner
    m = sn.extract(u, 0.0, *BOX)
    assert m["vertices"].shape == (1, 3) and m["triangles"].shape == (0, 3) and int(m["crossings"][0]) == 3
    np.testing.assert_array_equal(m["local"][0], np.float32([0.25, 0.25, 0.25]))  # (0.75 + 0 + 0) / 3 per axis
    np.testing.assert_array_equal(m["vertices"][0], np.float32([-0.5, -0.5, -0.5]))
    n = m["normals"][0]  # the gradient points into the corner: the normal away from it
    assert (n > 0).all() and abs(np.linalg.norm(n) - 1) < 1e-6
    # the other corner, and a box that is neither cubic nor centred
    u = np.full((2, 2, 2), -1.0, np.float32)
    u[1, 1, 1] = 1.0
    m = sn.extract(u, 0.0, [1.0, -2.0, 0.5], [3.0, -1.0, 4.5])
    np.testing.assert_array_equal(m["local"][0], np.float32([1, 1, 1]) - np.float32(0.5) / np.float32(3))
    want = (np.float32([1, 1, 1]) - np.float32(0.5) / np.float32(3)) / np.float32(1) * np.float32([2.0, 1.0, 4.0]) + np.float32([1.0, -2.0, 0.5])
    np.testing.assert_array_equal(m["vertices"][0], want)


def test_only_the_centre_inside_at_R_3_is_a_closed_octahedron_like_shell():
    u = np.full((3, 3, 3), -1.0, np.float32)
    u[1, 1, 1] = 1.0
    m = sn.extract(u, 0.0, *BOX)
    V, T = len(m["vertices"]), len(m["triangles"])
    assert (V, T) == (8, 12) and sorted(m["cells"]) == [(i * 3 + j) * 3 + k for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    c = sn.edge_census(m["triangles"])
    assert c["shared_twice"] and c["oriented"] and sn.euler(V, m["triangles"]) == 2 and sn.shells(V, m["triangles"]) == 1
    assert mr.signed_volume(m["vertices"], m["triangles"]) > 0
    assert sn.ambiguous_faces(u, 0.0) == 0 and sn.split_cells(u, 0.0) == 0
    # quads in ascending (p, a): the three edges into the centre (p = its lower neighbours, outside) then the three out of it
    centre = 13
    assert m["quad_edges"].tolist() == [[centre - 9, 0], [centre - 3, 1], [centre - 1, 2], [centre, 0], [centre, 1], [centre, 2]]


@pytest.mark.parametrize("kind,R,thresh", [("sphere", 9, 0.0), ("torus", 17, 0.0), ("random", 7, 0.0), ("random", 12, 0.25), ("plane", 9, 0.0),
                                           ("special", 9, 0.0), ("special", 17, 0.0), ("sphere", 12, 0.3)])
def test_the_counting_identities_and_the_vertex_inside_its_cell(kind, R, thresh):
    u = sn.field(kind, R, thresh)
    m = sn.extract(u, thresh, [-1.0, -2.0, 0.5], [3.0, -1.0, 4.5])
    ins = mr.inside(u, thresh)
    assert len(m["vertices"]) == int(sn.active_cells(ins).sum()) and (np.diff(m["cells"]) > 0).all()
    interior = 0
    for a in range(3):
        x = np.moveaxis(ins, a, 0)[:, 1:R - 1, 1:R - 1]
        interior += int((x[:-1] != x[1:]).sum())
    assert len(m["triangles"]) == 2 * interior == 2 * len(m["quads"])
    assert (m["crossings"] >= 3).all() and (m["crossings"] <= 12).all()
    finite = np.isfinite(m["local"]).all(axis=1)
    assert ((m["local"][finite] >= 0) & (m["local"][finite] <= 1)).all()  # exactly: no slack
    q = np.stack([m["cells"] // (R * R), (m["cells"] // R) % R, m["cells"] % R], axis=1)
    assert ((m["lattice"][finite] >= q[finite]) & (m["lattice"][finite] <= q[finite] + 1)).all()
    if kind != "special":
        assert finite.all()
    else:
        assert not finite.all() and finite.any()  # a NaN corner opposite an inside one gives a NaN vertex, as in pvd_hip_mesh.h
    if len(m["triangles"]):
        assert m["triangles"].min() >= 0 and m["triangles"].max() < len(m["vertices"])
        assert (m["quads"] >= 0).all()


def test_the_sequence_and_the_split_rules_on_quads_built_by_hand():
    sq = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    quad = [[0, 1, 2, 3]]
    short13 = sq.copy()
    short13[1], short13[3] = [0.75, 0.25, 0], [0.25, 0.75, 0]  # d13 = 0.5 < d02 = 2
    split, tri = sn.split_quads(short13, quad)
    assert split.tolist() == [True] and tri.tolist() == [[0, 1, 3], [1, 2, 3]]
    split, tri = sn.split_quads(sq, quad)  # d13 == d02: the first diagonal
    assert split.tolist() == [False] and tri.tolist() == [[0, 1, 2], [0, 2, 3]]
    for k in range(4):  # a NaN anywhere: the first diagonal
        bad = short13.copy()
        bad[k, 1] = np.nan
        split, tri = sn.split_quads(bad, quad)
        assert split.tolist() == [False] and tri.tolist() == [[0, 1, 2], [0, 2, 3]]
    # the sequence: the same crossing x edge with p inside and with p outside turns the quad round
    for sign, want in ((1.0, [0, 2, 3, 1]), (-1.0, [0, 1, 3, 2])):  # cells (0,0,0) (0,0,1) (0,1,0) (0,1,1) = vertices 0 1 2 3
        u = np.full((3, 3, 3), -sign, np.float32)
        u[0] = sign  # the layer i = 0 inside (sign > 0) or outside
        m = sn.extract(u, 0.0, *BOX)
        assert len(m["vertices"]) == 4 and m["quad_edges"].tolist() == [[4, 0]]  # p = (0,1,1), a = x: the only interior edge
        # q0 = p - e_y - e_z = cell 0, q1 = p - e_z = cell (0,1,0) = vertex 2, q2 = p = vertex 3, q3 = p - e_y = cell (0,0,1) = vertex 1
        assert m["quads"].tolist() == [want]
        nrm = np.cross(m["vertices"][m["triangles"][0, 1]] - m["vertices"][m["triangles"][0, 0]],
                       m["vertices"][m["triangles"][0, 2]] - m["vertices"][m["triangles"][0, 0]])
        assert nrm[0] * sign > 0 and nrm[1] == 0 and nrm[2] == 0  # from inside to outside


def test_nan_and_equality_are_outside_and_constant_fields_give_nothing():
    for kind in ("inside", "outside"):
        for thresh in (0.0, 0.5):
            m = sn.extract(sn.field(kind, 5, thresh), thresh, *BOX)
            assert m["vertices"].shape == (0, 3) and m["triangles"].shape == (0, 3) and m["normals"].shape == (0, 3)
    u = np.full((3, 3, 3), 0.5, np.float32)  # u == thresh everywhere: all outside
    assert len(sn.extract(u, 0.5, *BOX)["vertices"]) == 0
    u[1, 1, 1] = np.nan  # NaN is outside too
    assert len(sn.extract(u, 0.5, *BOX)["vertices"]) == 0
    u[1, 1, 1] = 1.0  # inside, every neighbour equal to thresh: t = (0.5 - 1) / (0.5 - 1) = 1 from the inside end, 0 from the other
    m = sn.extract(u, 0.5, *BOX)
    assert len(m["vertices"]) == 8 and np.isfinite(m["vertices"]).all()
    # the crossings sit ON the outside neighbours: cell (0,0,0) has them at (0,1,1), (1,0,1), (1,1,0) in local coordinates
    np.testing.assert_array_equal(m["local"][0], np.float32([2, 2, 2]) / np.float32(3))
    u[0, 1, 1] = np.nan  # an outside NaN end of a crossing edge: the four cells around it get NaN vertices
    m = sn.extract(u, 0.5, *BOX)
    assert int((~np.isfinite(m["vertices"]).all(axis=1)).sum()) == 4 and len(m["triangles"]) == 12
    # the (0,0,0) rule: a field whose gradient is zero at every stencil of the cell cannot be active; a zero MEAN gradient can
    u = np.full((3, 3, 3), -1.0, np.float32)
    u[1, 1, 1] = 1.0
    m = sn.extract(u, 0.0, [0, 0, 0], [1, 1, 1])
    assert (np.linalg.norm(m["normals"], axis=1) > 0.99).all()
    u = np.full((4, 4, 4), -1.0, np.float32)
    u[1:3, 1:3, 1:3] = np.inf  # gradients inf - inf and inf: len is not finite
    m = sn.extract(u, 0.0, *BOX)
    assert len(m["normals"]) > 0 and (m["normals"] == 0).all()


def test_a_non_cubic_shifted_box_moves_the_vertices_and_tilts_the_normals():
    u = sn.field("sphere", 9)
    a = sn.extract(u, 0.0, *BOX)
    lo, hi = np.float32([1.0, -2.0, 0.5]), np.float32([3.0, -1.0, 4.5])
    b = sn.extract(u, 0.0, lo, hi)
    np.testing.assert_array_equal(b["local"], a["local"])
    np.testing.assert_array_equal(b["vertices"], b["lattice"] / np.float32(8) * (hi - lo) + lo)
    assert np.array_equal(a["quads"], b["quads"]) and not np.array_equal(a["split"], b["split"])  # the diagonals are measured in the world
    # the normal is the gradient in world units: n_b ~ n_a scaled per axis by 1 / extent, renormalised
    w = a["normals"].astype(np.float64) * 2.0 / (hi - lo)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    assert np.abs(w - b["normals"]).max() < 1e-5


@pytest.mark.parametrize("kind", SMOOTH)
@pytest.mark.parametrize("R", SIZES)
def test_topology_where_no_face_is_ambiguous_and_no_cell_is_split(meshes, kind, R):
    u, m = meshes[kind, R]
    assert sn.ambiguous_faces(u, 0.0) == 0 and sn.split_cells(u, 0.0) == 0  # the condition of this test, not a measurement
    V = len(m["vertices"])
    c = sn.edge_census(m["triangles"])
    assert c["shared_twice"] and c["oriented"] and c["most"] == 2  # closed, every edge shared exactly twice, consistently wound
    assert sn.shells(V, m["triangles"]) == 1
    assert sn.euler(V, m["triangles"]) == (0 if kind == "torus" else 2)
    assert mr.signed_volume(m["vertices"], m["triangles"]) > 0


def test_an_ambiguous_face_is_counted_and_breaks_the_manifold_there_but_every_edge_stays_even():
    u = np.full((4, 4, 4), -1.0, np.float32)
    u[1, 1, 1] = u[1, 2, 2] = 1.0  # two inside points across a face diagonal
    assert sn.ambiguous_faces(u, 0.0) == 1 and sn.split_cells(u, 0.0) == 2
    m = sn.extract(u, 0.0, *BOX)
    c = sn.edge_census(m["triangles"])
    assert c["even"] and c["most"] == 4 and not c["shared_twice"]
    u = sn.field("random", 9)
    assert sn.ambiguous_faces(u, 0.0) > 100
    assert sn.edge_census(sn.extract(u, 0.0, *BOX)["triangles"])["most"] == 4
    # away from the box faces: every triangle edge between cells that do not touch the boundary layer is shared an even number of times
    R = 9
    m = sn.extract(u, 0.0, *BOX)
    q = np.stack([m["cells"] // (R * R), (m["cells"] // R) % R, m["cells"] % R], axis=1)
    inner = ((q >= 1) & (q <= R - 3)).all(axis=1)
    d = np.sort(mr.directed_edges(m["triangles"]), axis=1)
    d = d[inner[d[:, 0]] & inner[d[:, 1]]]
    assert len(d) > 1000 and (np.unique(d, axis=0, return_counts=True)[1] % 2 == 0).all()


@pytest.mark.parametrize("kind", ("sphere", "shifted"))
@pytest.mark.parametrize("R", (17, 33, 65))
def test_the_sphere_within_the_derived_bounds(meshes, kind, R):
    _, m = meshes[kind, R]
    centre = np.float64(sn.SHIFT if kind == "shifted" else (0, 0, 0))
    x = m["vertices"].astype(np.float64) - centre
    r = np.linalg.norm(x, axis=1)
    below, above = sn.sphere_position_bound(R)
    print("%s R=%d: |v| - 0.6 in [%.3e, %.3e], derived [-%.3e, +%.3e]" % (kind, R, (r - 0.6).min(), (r - 0.6).max(), below, above))
    assert (0.6 - r).max() <= below and (r - 0.6).max() <= above
    err = np.linalg.norm(m["normals"].astype(np.float64) - x / r[:, None], axis=1).max()
    bound = sn.sphere_normal_bound(R)
    print("%s R=%d: normals within %.3e of the analytic ones, derived %.3e" % (kind, R, err, bound))
    assert err <= bound
    assert R == 17 or bound < 0.1  # the bound says something from R = 33 on


def _nearest(a, b):
    """[len(a)]: the distance of every row of a to the nearest row of b (brute force, in blocks)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty(len(a))
    for s in range(0, len(a), 512):
        out[s:s + 512] = np.sqrt(((a[s:s + 512, None, :] - b[None, :, :]) ** 2).sum(axis=2).min(axis=1))
    return out


@pytest.mark.parametrize("kind,R", [("sphere", 17), ("shifted", 17), ("torus", 17), ("random", 9), ("sphere", 33)])
def test_against_marching_tetrahedra_within_one_cell_diagonal_both_ways(kind, R):
    """An active cell has a crossing axis edge, which carries a tetrahedra vertex in that cell; every crossing lattice edge of the Kuhn
    split (axis, face or body diagonal) lies in a cell whose corners differ, i.e. an active one, which carries a nets vertex; both stay in
    that cell, whose diameter is the cell diagonal."""
    u = sn.field(kind, R)
    lo, hi = [-1.0, -2.0, 0.5], [3.0, -1.0, 4.5]
    nets = sn.extract(u, 0.0, lo, hi, with_normals=False)["vertices"]
    tets = mr.extract(u, 0.0, lo, hi)[0]
    diagonal = float(np.linalg.norm((np.float64(hi) - np.float64(lo)) / (R - 1)))
    slack = 1e-6  # float32 positions of magnitude < 5
    assert len(nets) and len(tets) > len(nets)
    assert _nearest(nets, tets).max() <= diagonal + slack and _nearest(tets, nets).max() <= diagonal + slack


def test_float64_arithmetic_agrees_to_rounding_and_keeps_the_combinatorics():
    u = sn.field("torus", 17)
    a, b = sn.extract(u, 0.0, *BOX), sn.extract(u, 0.0, *BOX, dtype=np.float64)
    assert b["vertices"].dtype == np.float64 and np.array_equal(a["quads"], b["quads"]) and np.array_equal(a["cells"], b["cells"])
    assert np.abs(a["vertices"] - b["vertices"]).max() < 1e-6 and np.abs(a["normals"] - b["normals"]).max() < 1e-5
