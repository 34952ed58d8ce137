"""tests/mesh_restatement.py -- the numpy restatement of marching tetrahedra on the Kuhn split that tests/test_hip_mesh.py compares
the kernels with -- is pinned here on fields whose surfaces are known: closed, consistently wound, of the right genus, outward, on
their lattice edges, and converging to the sphere's volume and area.  No GPU, no library."""
import os

import numpy as np
import pytest

import mesh_restatement as mr

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def _mesh(u):
    owners, slots, tris = mr.topology(u, 0.0)
    world, t, lat = mr.positions(u, 0.0, owners, slots, BMIN, BMAX, np.float64)
    return dict(u=u, owners=owners, slots=slots, tris=tris, verts=world, t=t, lat=lat)


@pytest.fixture(scope="module")
def meshes():
    cut = mr.sphere_field(14, radius=0.6, centre=(0.7, 0.0, -0.8))  # leaves the box through the faces x = 1 and z = -1
    return {"sphere": _mesh(mr.sphere_field(12)), "torus": _mesh(mr.torus_field(16)), "two": _mesh(mr.two_spheres_field(16)),
            "cut": _mesh(cut)}


def _edge_census(tris):
    """{(a, b): count} over directed edges."""
    e = mr.directed_edges(tris)
    keys, counts = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(keys, counts)}


def _closed_and_consistent(tris):
    """Every edge is used by exactly two triangles, once in each direction."""
    census = _edge_census(tris)
    return all(c == 1 and census.get((b, a)) == 1 for (a, b), c in census.items())


def _euler(n_vertices, tris):
    e = mr.directed_edges(tris)
    und = np.unique(np.sort(e, axis=1), axis=0)
    return n_vertices - len(und) + len(tris)


def test_the_sphere_is_closed_consistently_wound_and_of_genus_zero(meshes):
    m = meshes["sphere"]
    assert len(m["tris"]) > 100
    assert _closed_and_consistent(m["tris"])
    assert _euler(len(m["verts"]), m["tris"]) == 2
    assert np.array_equal(np.unique(m["tris"]), np.arange(len(m["verts"])))  # every vertex is used, none is missing
    assert mr.signed_volume(m["verts"], m["tris"]) > 0


def test_the_torus_has_euler_characteristic_zero(meshes):
    m = meshes["torus"]
    assert _closed_and_consistent(m["tris"])
    assert _euler(len(m["verts"]), m["tris"]) == 0
    assert mr.signed_volume(m["verts"], m["tris"]) > 0


def test_two_disjoint_spheres_are_two_outward_components(meshes):
    m = meshes["two"]
    assert _closed_and_consistent(m["tris"])
    label = mr.components(len(m["verts"]), m["tris"])
    names = np.unique(label)
    assert len(names) == 2
    for name in names:
        part = m["tris"][label[m["tris"][:, 0]] == name]
        assert _closed_and_consistent(part) and _euler(int((label == name).sum()), part) == 2
        assert mr.signed_volume(m["verts"], part) > 0


def test_a_sphere_cut_by_the_box_is_open_only_on_box_faces(meshes):
    m = meshes["cut"]
    census = _edge_census(m["tris"])
    assert all(c == 1 for c in census.values())  # consistently wound: no directed edge twice
    boundary = [(a, b) for (a, b) in census if (b, a) not in census]
    assert boundary
    R = m["u"].shape[0]
    on_faces = set()
    for a, b in boundary:
        la, lb = m["lat"][a], m["lat"][b]
        faces = [(ax, side) for ax in range(3) for side in (0.0, R - 1.0) if la[ax] == side and lb[ax] == side]
        assert faces, (la, lb)
        on_faces.update(faces)
    assert on_faces == {(0, R - 1.0), (2, 0.0)}


@pytest.mark.parametrize("name", ["sphere", "torus", "two", "cut"])
def test_every_vertex_sits_on_its_edge_where_the_field_crosses_the_threshold(meshes, name):
    m = meshes[name]
    u, t = m["u"].reshape(-1).astype(np.float64), m["t"]
    R = m["u"].shape[0]
    assert np.all((t >= 0) & (t <= 1))
    d = np.asarray(mr.SLOTS)[m["slots"]]
    p = np.stack([m["owners"] // (R * R), (m["owners"] // R) % R, m["owners"] % R], axis=1)
    assert np.array_equal(m["lat"], p + d * t[:, None])  # on the segment p -> p + d
    assert np.all(p + d <= R - 1)
    ua, ub = u[m["owners"]], u[((p + d) @ np.array([R * R, R, 1]))]
    assert np.all((ua > 0) != (ub > 0))
    interp = ua + t * (ub - ua)
    assert np.all(np.abs(interp) <= 4 * np.finfo(np.float64).eps * (np.abs(ua) + np.abs(ub)))
    # the float32 positions are the float64 ones up to rounding, and the triangles do not depend on the arithmetic
    v32, tris32 = mr.extract(m["u"], 0.0, BMIN, BMAX, np.float32)
    assert v32.dtype == np.float32 and np.array_equal(tris32, m["tris"])
    assert np.abs(v32 - m["verts"]).max() <= 8 * np.finfo(np.float32).eps
    # order: vertices by (owner, slot), no duplicates
    key = m["owners"] * 7 + m["slots"]
    assert np.all(np.diff(key) > 0)


def test_nan_and_threshold_values_are_outside():
    u = np.full((3, 3, 3), -1.0, np.float32)
    u[1, 1, 1] = 1.0
    u[0, 0, 0] = np.nan
    u[2, 2, 2] = 0.0
    ins = mr.inside(u, 0.0)
    assert ins.sum() == 1 and ins[1, 1, 1]
    owners, slots, tris = mr.topology(u, 0.0)
    assert len(owners) == 14 and _closed_and_consistent(tris)  # the 14 lattice edges at the centre point
    assert mr.topology(np.ones((4, 4, 4), np.float32), 0.0)[2].shape == (0, 3)
    assert mr.topology(-np.ones((4, 4, 4), np.float32), 0.0)[2].shape == (0, 3)


def test_the_split_is_the_documented_one():
    assert mr.PERMS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    assert mr.TETS[0] == ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)) and mr.TETS[5] == ((0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1))
    # the six tetrahedra tile the cell: volumes 1/6 each
    for tet in mr.TETS:
        c = np.array(tet, float)
        assert abs(abs(np.linalg.det(c[1:] - c[0])) - 1.0) < 1e-12


def test_volume_and_area_converge_to_the_sphere():
    """r = 0.6: volume 4/3 pi r^3, area 4 pi r^2.  The errors at R = 12, 24, 48 decrease monotonically (no fixed tolerance); they are
    printed and kept in profiles/mesh_extract.txt."""
    r = 0.6
    vol, ar = 4.0 / 3.0 * np.pi * r ** 3, 4.0 * np.pi * r ** 2
    lines, ev, ea = [], [], []
    for R in (12, 24, 48):
        u = mr.sphere_field(R, r)
        verts, tris = mr.extract(u, 0.0, BMIN, BMAX, np.float64)
        ev.append(abs(mr.signed_volume(verts, tris) - vol) / vol)
        ea.append(abs(mr.area(verts, tris) - ar) / ar)
        lines.append("convergence sphere r=0.6 R=%d: V=%d T=%d rel. volume error %.6f rel. area error %.6f" % (R, len(verts), len(tris), ev[-1], ea[-1]))
        print(lines[-1])
    assert ev[0] > ev[1] > ev[2] and ea[0] > ea[1] > ea[2]
    path = os.path.join(REPO, "profiles", "mesh_extract.txt")
    try:
        old = open(path).read().splitlines() if os.path.exists(path) else []
        kept = [ln for ln in old if not ln.startswith("convergence ")]
        new = lines + kept
        if new != old:
            with open(path, "w") as f:
                f.write("\n".join(new) + "\n")
    except OSError:  # a read-only checkout: the figures were printed
        pass
