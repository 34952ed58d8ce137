"""Marching tetrahedra on the Kuhn split, restated in plain numpy from the description in include/pvd_hip_mesh.h (not from the
kernel): what csrc/mesh.hip is compared with in tests/test_hip_mesh.py, and what tests/test_mesh_restatement.py pins first.

Field u [R,R,R] f32, x-major.  Inside iff u > thresh (NaN, u == thresh: outside).  Every cell is cut into the 6 tetrahedra around
its diagonal, one per order of the axes (xyz, xzy, yxz, yzx, zxy, zyx), corners 0, e_a, e_a + e_b, (1,1,1).  Vertices sit on the
lattice edges p -> p + d, d one of SLOTS, whose endpoints differ, ordered by (owner's linear index, slot); triangles by (cell,
tetrahedron, triangle).  The winding is NOT taken from the header's parity rule: every triangle is turned so that its normal, taken
with the vertices at the edge midpoints (exact in integers), points from the inside corners' centroid to the outside corners'.
"""
import functools
import itertools

import numpy as np

SLOTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: xyz xzy yxz yzx zxy zyx


def tet_corners(perm):
    """The four corner offsets of the tetrahedron that walks the axes in the order `perm`."""
    c, out = [0, 0, 0], [(0, 0, 0)]
    for a in perm:
        c[a] = 1
        out.append(tuple(c))
    return out


TETS = tuple(tuple(tet_corners(p)) for p in PERMS)


def inside(u, thresh):
    with np.errstate(invalid="ignore"):
        return np.asarray(u, np.float32) > np.float32(thresh)


def _vertices(ins):
    """(owner linear index, slot) of every vertex, in order."""
    R = ins.shape[0]
    lin = np.arange(R ** 3, dtype=np.int64).reshape(R, R, R)
    owners, slots = [], []
    for s, (dx, dy, dz) in enumerate(SLOTS):
        a = ins[:R - dx, :R - dy, :R - dz]
        b = ins[dx:, dy:, dz:]
        own = lin[:R - dx, :R - dy, :R - dz][a != b]
        owners.append(own)
        slots.append(np.full(own.shape, s, np.int64))
    owners, slots = np.concatenate(owners), np.concatenate(slots)
    order = np.lexsort((slots, owners))
    return owners[order], slots[order]


def _turn(tri_offsets, in_corners, out_corners):
    """True when the triangle through the midpoints of the edges `tri_offsets` = [(ca, cb)] * 3 must exchange two vertices for its
    normal to point from the inside corners to the outside corners (all in doubled integer coordinates)."""
    p = [np.array(ca) + np.array(cb) for ca, cb in tri_offsets]
    nrm = np.cross(p[1] - p[0], p[2] - p[0])
    d = np.sum(out_corners, axis=0) * len(in_corners) - np.sum(in_corners, axis=0) * len(out_corners)
    s = int(np.dot(nrm, d))
    assert s != 0
    return s < 0


@functools.lru_cache(maxsize=None)
def _tet_triangles(ti, state):
    """The triangles of tetrahedron `ti` whose corners 0..3 are inside where `state` says so: a list of triangles, each three
    edges (corner offset, corner offset) of the cell, wound outwards."""
    corners = TETS[ti]
    n_in = sum(state)
    if n_in in (0, 4):
        return []
    ins_c = [q for q in range(4) if state[q]]
    out_c = [q for q in range(4) if not state[q]]

    def edge(x, y):
        return (corners[min(x, y)], corners[max(x, y)])
    if n_in == 2:
        (A, B), (C, D) = ins_c, out_c
        cand = [[edge(A, C), edge(A, D), edge(B, D)], [edge(A, C), edge(B, D), edge(B, C)]]
    else:
        A = ins_c[0] if n_in == 1 else out_c[0]
        B, C, D = [q for q in range(4) if q != A]
        cand = [[edge(A, B), edge(A, C), edge(A, D)]]
    out = []
    for t in cand:
        if _turn(t, [corners[q] for q in ins_c], [corners[q] for q in out_c]):
            t = [t[0], t[2], t[1]]
        out.append(t)
    return out


def topology(u, thresh):
    """owners [V], slots [V] (int64) and triangles [T,3] (int32) of the level set u = thresh."""
    u = np.asarray(u, np.float32)
    R = u.shape[0]
    assert u.shape == (R, R, R) and R >= 2
    ins = inside(u, thresh)
    owners, slots = _vertices(ins)
    index = {(int(o), int(s)): n for n, (o, s) in enumerate(zip(owners, slots))}
    slot_of = {d: s for s, d in enumerate(SLOTS)}

    def vertex(p, ca, cb):  # the vertex on the edge between the corners ca, cb (ca before cb on the walk) of the cell at p
        own = ((p[0] + ca[0]) * R + p[1] + ca[1]) * R + p[2] + ca[2]
        return index[(own, slot_of[(cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2])])]

    # cells whose 8 corners do not agree, in linear order (the others have no triangle)
    c = ins.astype(np.int8)
    tot = sum(c[dx:R - 1 + dx, dy:R - 1 + dy, dz:R - 1 + dz] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    tris = []
    for p in np.argwhere((tot > 0) & (tot < 8)):
        p = tuple(int(v) for v in p)
        for ti, corners in enumerate(TETS):
            state = tuple(bool(ins[p[0] + o[0], p[1] + o[1], p[2] + o[2]]) for o in corners)
            for t in _tet_triangles(ti, state):
                tris.append([vertex(p, ca, cb) for ca, cb in t])
    return owners, slots, np.asarray(tris, np.int32).reshape(-1, 3)


def positions(u, thresh, owners, slots, bmin, bmax, dtype=np.float32):
    """World positions [V,3] in `dtype` arithmetic, operation by operation as the header states them, the interpolation
    parameters t [V], and the lattice positions [V,3].  The inputs are the SAME float32 numbers for both dtypes."""
    u = np.asarray(u, np.float32)
    R = u.shape[0]
    d = np.asarray(SLOTS, np.int64)[slots]
    p = np.stack([owners // (R * R), (owners // R) % R, owners % R], axis=1)
    other = ((p[:, 0] + d[:, 0]) * R + p[:, 1] + d[:, 1]) * R + p[:, 2] + d[:, 2]
    flat = u.reshape(-1)
    ua, ub, th = flat[owners].astype(dtype), flat[other].astype(dtype), dtype(np.float32(thresh))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (th - ua) / (ub - ua)
        pf = p.astype(dtype)
        lat = np.where(d == 1, pf + t[:, None], pf)
        lo, hi = np.asarray(bmin, np.float32).astype(dtype), np.asarray(bmax, np.float32).astype(dtype)
        world = lat / dtype(R - 1) * (hi - lo)[None, :] + lo[None, :]
    assert world.dtype == dtype
    return world, t, lat


def extract(u, thresh, bmin, bmax, dtype=np.float32):
    """(vertices [V,3] dtype, triangles [T,3] int32)."""
    owners, slots, tris = topology(u, thresh)
    return positions(u, thresh, owners, slots, bmin, bmax, dtype)[0], tris


# ------------------------------------------------------------------ fields the tests share (box [-1,1]^3 unless stated)
def grid(R, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, R)
    return np.meshgrid(x, x, x, indexing="ij")


def sphere_field(R, radius=0.6, centre=(0.0, 0.0, 0.0), lo=-1.0, hi=1.0):
    """radius - |x - c|: positive inside; threshold 0."""
    X, Y, Z = grid(R, lo, hi)
    return (radius - np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2)).astype(np.float32)


def torus_field(R, major=0.55, minor=0.25):
    X, Y, Z = grid(R)
    return (minor - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - major) ** 2 + Z ** 2)).astype(np.float32)


def two_spheres_field(R, radius=0.3, c0=(-0.5, -0.45, -0.4), c1=(0.5, 0.45, 0.4)):
    return np.maximum(sphere_field(R, radius, c0), sphere_field(R, radius, c1))


# ------------------------------------------------------------------ mesh measures
def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def area(verts, tris):
    v = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    return float(np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum() / 2.0)


def components(n_vertices, tris):
    """Label of the connected component of every vertex (union-find over triangle edges)."""
    parent = np.arange(n_vertices)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in directed_edges(tris):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(a) for a in range(n_vertices)])
