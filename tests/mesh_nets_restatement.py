"""Naive surface nets, restated in vectorised numpy from the description in csrc/pvd_hip_mesh_nets.h (not from the kernel): what
csrc/mesh_nets.hip is compared with in tests/test_hip_mesh_nets.py, and what tests/test_mesh_nets_restatement.py pins first.

Field u [R,R,R] f32, x-major.  Inside iff u > thresh.  A cell is active iff its 8 corners do not agree; its vertex is the mean of the
crossings of its 12 edges e = 4a + 2 o_b + o_c (b = (a+1)%3, c = (a+2)%3), summed in ascending e, at t = (thresh - u_A) / (u_B - u_A);
vertices in ascending cell index.  Every crossing interior lattice edge p -> p + e_a emits the quad over the cells p - e_b - e_c, p - e_c,
p, p - e_b (the other way round when p is outside), split along the shorter diagonal of the emitted positions (the first on ties and
NaN); triangles in ascending (p, a).  Normals: the mean over the same crossings of the interpolated lattice gradient of
mesh_normals_restatement.lattice_gradient, negated and normalised.  Every operation is one numpy operation of `dtype`, so rounded on its
own; the inputs are the SAME float32 numbers for both dtypes.
"""
import numpy as np

import mesh_normals_restatement as nr
import mesh_restatement as mr

CELL_EDGES = 12


def _axis_bit(a):
    return 4 >> a


def edge_ends(e):
    """(a, o_b, o_c, corner code of A, corner code of B); a corner code is ox * 4 + oy * 2 + oz."""
    a, ob, oc = e >> 2, (e >> 1) & 1, e & 1
    A = ob * _axis_bit((a + 1) % 3) + oc * _axis_bit((a + 2) % 3)
    return a, ob, oc, A, A | _axis_bit(a)


def _corner(x, c):
    """The view of the lattice array x [R,R,R,...] at corner c of every cell: [R-1,R-1,R-1,...]."""
    R = x.shape[0]
    ox, oy, oz = c >> 2, (c >> 1) & 1, c & 1
    return x[ox:R - 1 + ox, oy:R - 1 + oy, oz:R - 1 + oz]


def active_cells(ins):
    """[R-1,R-1,R-1] bool."""
    tot = sum(_corner(ins, c).astype(np.int8) for c in range(8))
    return (tot > 0) & (tot < 8)


def extract(u, thresh, bmin, bmax, dtype=np.float32, with_normals=True):
    """dict(vertices [V,3] dtype, triangles [T,3] int32, normals [V,3] dtype or None, cells [V] int64 (the cell's linear index),
    local [V,3] dtype (m, the position inside the cell), lattice [V,3] dtype, quads [T/2,4] int64 (k0..k3), quad_edges [T/2,2] int64
    (p's linear index, a), split [T/2] bool (True: the diagonal k1-k3 was taken))."""
    u = np.asarray(u, np.float32)
    R = u.shape[0]
    assert u.shape == (R, R, R) and R >= 2
    ins = mr.inside(u, thresh)
    th = dtype(np.float32(thresh))
    lo, hi = np.asarray(bmin, np.float32).astype(dtype), np.asarray(bmax, np.float32).astype(dtype)
    act = active_cells(ins)
    q = np.argwhere(act)  # lexicographic in (i, j, k): ascending cell index
    V = len(q)
    cells = (q[:, 0] * R + q[:, 1]) * R + q[:, 2]
    uc = [_corner(u, c)[act].astype(dtype) for c in range(8)]
    inc = [_corner(ins, c)[act] for c in range(8)]
    if with_normals:
        g = nr.lattice_gradient(u, dtype(R - 1) / (hi - lo), dtype)
        gc = [_corner(g, c)[act] for c in range(8)]
        G = np.zeros((V, 3), dtype)
    s = np.zeros((V, 3), dtype)
    count = np.zeros(V, np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for e in range(CELL_EDGES):
            a, ob, oc, A, B = edge_ends(e)
            cross = inc[A] != inc[B]
            t = (th - uc[A]) / (uc[B] - uc[A])
            l = np.empty((V, 3), dtype)
            l[:, a], l[:, (a + 1) % 3], l[:, (a + 2) % 3] = t, dtype(ob), dtype(oc)
            s = np.where(cross[:, None], s + l, s)
            count += cross
            if with_normals:
                Ge = gc[A] + t[:, None] * (gc[B] - gc[A])
                G = np.where(cross[:, None], G + Ge, G)
        cnt = count.astype(dtype)
        m = s / cnt[:, None]
        lattice = q.astype(dtype) + m
        vertices = lattice / dtype(R - 1) * (hi - lo)[None, :] + lo[None, :]
        normals = None
        if with_normals:
            G = G / cnt[:, None]
            length = np.sqrt(G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1] + G[:, 2] * G[:, 2])
            ok = np.isfinite(length) & (length > 0)
            normals = np.where(ok[:, None], -G / length[:, None], dtype(0))
    assert vertices.dtype == dtype and m.dtype == dtype

    # ---- quads
    index = np.full(R ** 3, -1, np.int64)
    index[cells] = np.arange(V)
    stride = (R * R, R, 1)
    lin = np.arange(R ** 3, dtype=np.int64).reshape(R, R, R)
    ps, axes, insides = [], [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        sl_p, sl_n = [None] * 3, [None] * 3
        sl_p[a], sl_n[a] = slice(0, R - 1), slice(1, R)
        sl_p[b] = sl_n[b] = slice(1, R - 1)
        sl_p[c] = sl_n[c] = slice(1, R - 1)
        sl_p, sl_n = tuple(sl_p), tuple(sl_n)
        cross = ins[sl_p] != ins[sl_n]
        ps.append(lin[sl_p][cross])
        axes.append(np.full(len(ps[-1]), a, np.int64))
        insides.append(ins[sl_p][cross])
    ps, axes, insides = np.concatenate(ps), np.concatenate(axes), np.concatenate(insides)
    order = np.lexsort((axes, ps))
    ps, axes, insides = ps[order], axes[order], insides[order]
    sb, sc = np.asarray(stride)[(axes + 1) % 3], np.asarray(stride)[(axes + 2) % 3]
    q0, q1, q2, q3 = index[ps - sb - sc], index[ps - sc], index[ps], index[ps - sb]
    assert (np.stack([q0, q1, q2, q3]) >= 0).all()  # all four cells are active: each contains the edge
    quads = np.stack([q0, np.where(insides, q1, q3), q2, np.where(insides, q3, q1)], axis=1)
    split, triangles = split_quads(vertices, quads)
    return dict(vertices=vertices, triangles=triangles, normals=normals, cells=cells, local=m, lattice=lattice, quads=quads,
                quad_edges=np.stack([ps, axes], axis=1), split=split, crossings=count)


def split_quads(vertices, quads):
    """(split [Q] bool, triangles [2Q,3] int32): d13 < d02 -> (k0,k1,k3), (k1,k2,k3); otherwise, ties and NaN too, (k0,k1,k2), (k0,k2,k3).
    The squared lengths in the dtype of `vertices`: differences, three products, (dx*dx + dy*dy) + dz*dz."""
    quads = np.asarray(quads, np.int64).reshape(-1, 4)
    P = vertices[quads]  # [Q,4,3]
    with np.errstate(invalid="ignore", over="ignore"):
        d = P[:, 2] - P[:, 0]
        d02 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d = P[:, 3] - P[:, 1]
        d13 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        split = d13 < d02
    k0, k1, k2, k3 = quads.T
    first = np.stack([k0, k1, np.where(split, k3, k2)], axis=1)
    second = np.stack([np.where(split, k1, k0), k2, k3], axis=1)
    return split, np.stack([first, second], axis=1).reshape(-1, 3).astype(np.int32)


# ------------------------------------------------------------------ what the topology tests are conditioned on
def ambiguous_faces(u, thresh):
    """The number of lattice faces with exactly their two diagonal corners inside."""
    ins = mr.inside(np.asarray(u, np.float32), thresh)
    R = ins.shape[0]
    n = 0
    for a in range(3):
        x = np.moveaxis(ins, a, 0)  # the face is spanned by the two other axes
        c00, c01, c10, c11 = x[:, :R - 1, :R - 1], x[:, :R - 1, 1:], x[:, 1:, :R - 1], x[:, 1:, 1:]
        n += int(((c00 == c11) & (c01 == c10) & (c00 != c01)).sum())
    return n


def _parts(mask):
    """The number of connected components of the corners in `mask` (bit = corner code) under the cube's edges."""
    todo, parts = {c for c in range(8) if (mask >> c) & 1}, 0
    while todo:
        parts += 1
        stack = [todo.pop()]
        while stack:
            c = stack.pop()
            for bit in (1, 2, 4):
                if (c ^ bit) in todo:
                    todo.remove(c ^ bit)
                    stack.append(c ^ bit)
    return parts


SPLIT_TABLE = np.array([_parts(m) > 1 or _parts(~m & 255) > 1 for m in range(256)])


def split_cells(u, thresh):
    """The number of cells whose inside corners, or whose outside corners, fall apart under the cube's edges."""
    ins = mr.inside(np.asarray(u, np.float32), thresh)
    mask = sum(_corner(ins, c).astype(np.int64) << c for c in range(8))
    return int(SPLIT_TABLE[mask].sum())


# ------------------------------------------------------------------ mesh measures
def edge_census(triangles):
    """dict(edges, shared_twice: every undirected edge is used by exactly two triangles, oriented: no directed edge is used twice,
    most: the largest number of triangles on one edge)."""
    d = mr.directed_edges(triangles)
    und = np.sort(d, axis=1)
    _, n = np.unique(und, axis=0, return_counts=True)
    _, nd = np.unique(d, axis=0, return_counts=True)
    return dict(edges=len(n), shared_twice=bool((n == 2).all()), oriented=bool((nd == 1).all()), most=int(n.max()) if len(n) else 0,
                even=bool((n % 2 == 0).all()))


def euler(n_vertices, triangles):
    return n_vertices - edge_census(triangles)["edges"] + len(triangles)


def shells(n_vertices, triangles):
    return len(np.unique(mr.components(n_vertices, triangles)))


def smallest_angles(vertices, triangles):
    """[T] degrees, float64."""
    p = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    out = np.full(len(p), 180.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(3):
            a, b = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
            c = np.einsum("ij,ij->i", a, b) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
            out = np.minimum(out, np.degrees(np.arccos(np.clip(np.nan_to_num(c, nan=1.0), -1.0, 1.0))))
    return out


# ------------------------------------------------------------------ fields the tests share (box [-1,1]^3 unless stated)
SHIFT = (0.07, -0.03, 0.11)


def field(kind, R, thresh=0.0):
    """The surface is the level set `thresh`."""
    thresh = np.float32(thresh)
    if kind == "sphere":
        u = mr.sphere_field(R)
    elif kind == "shifted":
        u = mr.sphere_field(R, centre=SHIFT)
    elif kind == "torus":
        u = mr.torus_field(R)
    elif kind == "random":  # nearly every cell is active, and ambiguous faces abound
        u = np.random.RandomState(R).uniform(-1, 1, (R, R, R)).astype(np.float32)
    elif kind == "plane":  # leaves through the box faces: boundary edges emit nothing
        X, Y, Z = mr.grid(R)
        u = (0.31 * X - 0.52 * Y + 0.8 * Z + 0.05).astype(np.float32)
    elif kind == "special":  # NaN, +-inf and values equal to thresh in a smooth field
        u = nr.smooth_field(R, 5)
        pick = np.random.RandomState(100 + R).uniform(size=u.shape)
        u[pick < 0.03] = np.nan
        u[(pick >= 0.03) & (pick < 0.05)] = np.inf
        u[(pick >= 0.05) & (pick < 0.07)] = -np.inf
        u[(pick >= 0.07) & (pick < 0.12)] = 0.0
    elif kind == "inside":
        u = np.full((R, R, R), 1.0, np.float32)
    elif kind == "outside":
        u = np.full((R, R, R), -1.0, np.float32)
    else:
        raise KeyError(kind)
    return (u + thresh).astype(np.float32)


# ------------------------------------------------------------------ derived bounds on the sphere u = r0 - |x|, box [-1,1]^3
def sphere_position_bound(R, r0=0.6):
    """(below, above): r0 - |v| <= below and |v| - r0 <= above for every vertex v.  u is 1-Lipschitz and |u''| <= 1 / |x| along a line.
    With h the lattice spacing, every point of an active cell is at least r0 - sqrt(3) h from the centre (the cell holds a point of the
    sphere and has diameter sqrt(3) h).  Linear interpolation of u on an axis edge of length h is off by at most e1 = h^2 / (8 (r0 -
    sqrt(3) h)), so the crossing, where the interpolant vanishes, has |u| = | r0 - |x| | <= e1.  The vertex is a mean of points with
    |x| <= r0 + e1, so it is no further out than that (a ball is convex).  All of them lie in the cell, i.e. within c / 2 of its centre z,
    c = sqrt(3) h, and have |x| >= rho = r0 - e1:  x . z = (|x|^2 + |z|^2 - |x - z|^2) / 2 >= (rho^2 + |z|^2 - c^2 / 4) / 2, the same
    holds for their mean, and (rho^2 - c^2 / 4 + d^2) / (2 d) >= sqrt(rho^2 - c^2 / 4) for every d = |z| > 0: the mean is at most the
    sagitta of a chord c of the sphere of radius rho below rho.  float32: the field is rounded once (2^-24, and u is 1-Lipschitz); the
    chain t, 12 sums, the division, q + m, / (R-1), * extent, + bmin is 17 roundings of lattice coordinates below 128, 2^-17 each at the
    most, times h."""
    h = 2.0 / (R - 1)
    assert r0 - np.sqrt(3.0) * h > 0
    e1 = h * h / (8.0 * (r0 - np.sqrt(3.0) * h))
    rho = r0 - e1
    slack = 2.0 ** -24 + 17 * 2.0 ** -17 * h
    return r0 - np.sqrt(rho * rho - 0.75 * h * h) + slack, e1 + slack


def sphere_normal_bound(R, r0=0.6):
    """| n - v / |v| | <= this for every vertex v.  For f = |x|: D^3 f [a,b,c] = -(P_ab x_c + P_ac x_b + P_bc x_a) / |x|^2 with
    P = I - x x^T / |x|^2 and x the unit vector, so |D^3 f| <= 3 / |x|^2.  Every point the stencils touch is within h of a corner of an
    active cell: |x| >= rho = r0 - (sqrt(3) + 1) h.  A central difference is off by at most h^2 / 6 * 3 / rho^2 per axis, linear
    interpolation of a gradient component along an edge by h^2 / 8 * 3 / rho^2: G_e is within sqrt(3) * (7 / 8) h^2 / rho^2 of grad u
    = -x / |x| at the crossing x_e.  x_e / |x_e| is within e1 / r0 of x_e / r0 (| r0 - |x_e| | <= e1), so the mean of them is within
    e1 / r0 of v / r0, which is within | |v| - r0 | / r0 <= below / r0 of v / |v|.  So -G = v / |v| + E, |E| <= eps, and normalising a
    vector within eps of a unit vector moves it by at most eps more.  float32: 1e-5 (tests/test_hip_mesh_normals.py bounds the chain by
    a few 2^-24 times gradient magnitudes of order 1)."""
    h = 2.0 / (R - 1)
    rho = r0 - (np.sqrt(3.0) + 1.0) * h
    assert rho > 0
    below, above = sphere_position_bound(R, r0)
    e1 = above
    eps = np.sqrt(3.0) * 0.875 * h * h / (rho * rho) + e1 / r0 + max(below, above) / r0
    return 2.0 * eps + 1e-5
