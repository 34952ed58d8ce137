"""numpy restatement of csrc/pvd_hip_mesh_tsdf.h: pvd_mesh_tsdf_integrate, pvd_mesh_tsdf_finalize and pvd_mesh_tsdf_sample_color,
operation for operation in the order the header writes them.  Every array and every scalar that takes part is of ONE dtype, so nothing
is promoted: dtype=np.float32 is the restatement the kernels are compared with bit for bit, dtype=np.float64 is its twin -- the same
decisions and the same order on the same float32 inputs, every operation in float64 -- used for the geometry check and as the
reference of the rounding bound.  Views are looped over in ascending order; voxels are vectorised (numpy rounds every elementwise
operation on its own and fuses nothing; its division and square root are correctly rounded).

Also here, because the CPU tests and the GPU tests share them: the analytic sphere fixture and the hand-made views of the skip rules."""
import numpy as np

MAX_R = 1024
MAX_SIDE = 16384


def lattice(R, bmin, bmax, dtype=np.float32):
    """p [R^3,3]: c_a(n) = (float)n / (float)(R - 1) * (hi_a - lo_a) + lo_a, x-major, z fastest."""
    lo, hi = np.asarray(bmin, np.float32).astype(dtype), np.asarray(bmax, np.float32).astype(dtype)
    n = np.arange(R).astype(dtype)
    axes = [n / dtype(R - 1) * (hi[a] - lo[a]) + lo[a] for a in range(3)]
    i, j, k = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    return np.stack([axes[0][i.ravel()], axes[1][j.ravel()], axes[2][k.ravel()]], axis=1)


def integrate(acc_d, acc_w, acc_c, depth, color, weight, poses, intrinsics, R, bmin, bmax, tau, dtype=np.float32, trace=None):
    """acc_d [R^3], acc_w [R^3], acc_c [R^3,3] or None (arrays of `dtype`, changed in place) += the views.  depth [V,H,W], color
    [V,H,W,3] or None, weight [V,H,W] or None, poses [V,4,4], intrinsics [V,4]: float32 arrays.  trace: a list that receives, per
    view, dict(x, y, qz, s, r, in_view, has_depth, kept) over all voxels (numbers are garbage where an earlier test already skipped the
    voxel; in_view, has_depth and kept are the masks after the image test, the depth test and the last test)."""
    V, H, W = depth.shape
    p = lattice(R, bmin, bmax, dtype)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    tau = dtype(np.float32(tau))
    fW, fH, one, zero = dtype(W), dtype(H), dtype(1), dtype(0)
    with_color = color is not None and acc_c is not None
    with np.errstate(all="ignore"):
        for v in range(V):
            M = poses[v].astype(np.float32).astype(dtype)
            fx, fy, cx, cy = intrinsics[v].astype(np.float32).astype(dtype)
            dx, dy, dz = px - M[0, 3], py - M[1, 3], pz - M[2, 3]
            qx = (M[0, 0] * dx + M[1, 0] * dy) + M[2, 0] * dz
            qy = (M[0, 1] * dx + M[1, 1] * dy) + M[2, 1] * dz
            qz = (M[0, 2] * dx + M[1, 2] * dy) + M[2, 2] * dz
            keep = qz > zero
            x = (fx * qx) / qz + cx
            y = (fy * qy) / qz + cy
            keep &= (x >= zero) & (x < fW) & (y >= zero) & (y < fH)
            in_view = keep.copy()
            i = np.where(keep, np.floor(x), zero).astype(np.int64)
            j = np.where(keep, np.floor(y), zero).astype(np.int64)
            D = depth[v][j, i].astype(dtype)
            keep &= D > zero
            has_depth = keep.copy()
            r = np.sqrt((dx * dx + dy * dy) + dz * dz)
            s = D - r
            keep &= s >= -tau
            t = np.minimum(s / tau, one)
            if weight is not None:
                w = weight[v][j, i].astype(dtype)
                keep &= (w > zero) & (w < dtype(np.inf))
            else:
                w = np.ones_like(t)
            acc_d[keep] = (acc_d + w * t)[keep]
            acc_w[keep] = (acc_w + w)[keep]
            if with_color:
                rgb = color[v][j, i].astype(dtype)
                acc_c[keep] = (acc_c + w[:, None] * rgb)[keep]
            if trace is not None:
                trace.append(dict(x=x, y=y, qz=qz, s=s, r=r, in_view=in_view, has_depth=has_depth, kept=keep.copy()))


def finalize(acc_d, acc_w, min_weight, unknown, dtype=np.float32):
    """(field [R^3], totals (observed, observed with field <= 0, unknown))"""
    with np.errstate(all="ignore"):
        seen = acc_w >= dtype(np.float32(min_weight))
        f = np.maximum(np.minimum(acc_d / acc_w, dtype(1)), dtype(-1))
    field = np.where(seen, f, dtype(np.float32(unknown))).astype(dtype)
    return field, (int(seen.sum()), int((seen & (field <= 0)).sum()), int((~seen).sum()))


def sample_color(acc_c, acc_w, R, bmin, bmax, min_weight, points, dtype=np.float32):
    """colors [N,3] of points [N,3] (float32)"""
    lo, hi = np.asarray(bmin, np.float32).astype(dtype), np.asarray(bmax, np.float32).astype(dtype)
    P = np.asarray(points, np.float32).astype(dtype)
    N = P.shape[0]
    r1, zero, one = dtype(R - 1), dtype(0), dtype(1)
    mw = dtype(np.float32(min_weight))
    in_box = np.ones(N, bool)
    base, f, g = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            u = (P[:, a] - lo[a]) / (hi[a] - lo[a]) * r1
            ok = (u >= zero) & (u <= r1)
            in_box &= ok
            cell = np.minimum(np.where(ok, np.floor(u), zero).astype(np.int64), R - 2)
            base.append(cell)
            fa = u - cell.astype(dtype)
            f.append(fa)
            g.append(one - fa)
        m_sum = np.zeros(N, dtype)
        c_sum = np.zeros((N, 3), dtype)
        for code in range(8):
            a, b, c = code >> 2, (code >> 1) & 1, code & 1
            n = ((base[0] + a) * R + (base[1] + b)) * R + (base[2] + c)
            w = acc_w[n]
            seen = in_box & (w >= mw)
            m = ((f[0] if a else g[0]) * (f[1] if b else g[1])) * (f[2] if c else g[2])
            m_sum = np.where(seen, m_sum + m, m_sum)
            c_sum = np.where(seen[:, None], c_sum + m[:, None] * (acc_c[n] / w[:, None]), c_sum)
        out = np.minimum(np.maximum(c_sum / m_sum[:, None], zero), one)
    return np.where((in_box & (m_sum > zero))[:, None], out, zero).astype(dtype)


# --------------------------------------------------------------------------------------------------------- shared fixtures
def observed_corners(acc_w, R, min_weight):
    """[R-1,R-1,R-1] int: how many of the 8 corners of every lattice cell are observed (acc_w >= min_weight)"""
    seen = (np.asarray(acc_w).reshape(R, R, R) >= min_weight).astype(np.int64)
    return sum(seen[a:R - 1 + a, b:R - 1 + b, c:R - 1 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1))


def single_corner_case():
    """A volume with ONE observed voxel -- the centre (2, 2, 2) of an R = 5 lattice over the box +-1, at the origin, acc_w = 2 and
    acc_c = (0.5, 1, 1.625), i.e. the colour (0.25, 0.5, 0.8125) -- and points in all 8 cells around it, each of which has exactly one
    observed corner: near the voxel, in the middle of the cell, close to the OPPOSITE corner (a trilinear weight of about 1e-9 and of
    about 2^-60: the renormalisation divides by that one small weight) and exactly on the opposite corner (the weight is 0: colour 0).
    Returns dict(R, bmin, bmax, acc_w [125], acc_c [125,3], color [3], points [8*5,3], exact_zero [8*5] bool)."""
    R = 5
    acc_w, acc_c = np.zeros(R ** 3, np.float32), np.zeros((R ** 3, 3), np.float32)
    n = (2 * R + 2) * R + 2
    acc_w[n], acc_c[n] = 2.0, (0.5, 1.0, 1.625)
    pts, zero = [], []
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                s = np.array([sx, sy, sz])
                for f in (0.05, 0.5, 0.4995, 0.5 * (1 - 2.0 ** -20), 0.5):  # distance from the voxel along each axis; the cell edge is 0.5
                    pts.append(s * f)
                    zero.append(False)
                pts[-4] = s * np.array([0.1, 0.25, 0.4])  # an uneven one in place of the second
                zero[-1] = True
    return dict(R=R, bmin=np.full(3, -1.0, np.float32), bmax=np.full(3, 1.0, np.float32), acc_w=acc_w, acc_c=acc_c,
                color=np.array([0.25, 0.5, 0.8125], np.float32), points=np.array(pts, np.float32), exact_zero=np.array(zero))


def look_at(c):
    """cam2world [4,4] f32 of a camera at c that looks at the origin along its +z (pvd/scene.py: get_rays' convention)."""
    c = np.asarray(c, np.float64)
    f = -c / np.linalg.norm(c)
    helper = np.array([0.0, 0.0, 1.0]) if abs(f[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    r = np.cross(helper, f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = r, u, f, c
    return M.astype(np.float32)


def sphere_cameras(n=14, distance=3.2):
    """the 6 axis views and, for n = 14, the 8 corner views, at `distance` from the origin"""
    axis = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    corner = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    dirs = np.array(axis + (corner if n == 14 else []), np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return np.stack([look_at(d * distance) for d in dirs])


def sphere_depth(poses, intrinsics, H, W, radius=0.5):
    """depth [V,H,W] f32: the exact distance along the unit ray through every pixel CENTRE to the sphere of `radius` about the origin
    (evaluated in float64 from the float32 cameras, rounded once), +inf where the ray misses it."""
    out = np.empty((len(poses), H, W), np.float32)
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    for v, (M, K) in enumerate(zip(poses.astype(np.float64), intrinsics.astype(np.float64))):
        d = np.stack([(ii - K[2]) / K[0], (jj - K[3]) / K[1], np.ones_like(ii)], axis=-1)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        d = d @ M[:3, :3].T
        o = M[:3, 3]
        b = d @ o
        disc = b * b - (o @ o - radius * radius)
        with np.errstate(invalid="ignore"):
            t = -b - np.sqrt(disc)
        out[v] = np.where(disc > 0, t, np.inf)
    return out


def sphere_fixture(R=33, HW=64, n=14, focal=None):
    """The analytic sphere of the geometry check: radius 0.5, box +-1, n cameras at distance 3.2, HW x HW exact depth maps, tau = 3
    lattice spacings.  The focal length (HW pixels across a field of view with tan(half) = 0.5) lets every axis view cover the whole box
    (its nearest face is 2.2 away and 1 wide each way), so no voxel is left to `unknown` for want of a camera.  The principal point is
    at a PIXEL CENTRE (HW / 2 - 0.5): the symmetry planes of the lattice contain the optical axes, and with the principal point on a
    pixel boundary every voxel of those planes would choose its pixel by the last bit of x."""
    focal = float(HW) if focal is None else float(focal)
    poses = sphere_cameras(n)
    intrinsics = np.tile(np.array([focal, focal, HW / 2 - 0.5, HW / 2 - 0.5], np.float32), (len(poses), 1))
    depth = sphere_depth(poses, intrinsics, HW, HW)
    # a colour per pixel that depends on the view and the pixel, so that a wrong gather shows
    v, j, i = np.meshgrid(np.arange(len(poses)), np.arange(HW), np.arange(HW), indexing="ij")
    color = np.stack([(i + 0.5) / HW, (j + 0.5) / HW, (v + 0.5) / len(poses)], axis=-1).astype(np.float32)
    spacing = 2.0 / (R - 1)
    return dict(R=R, bmin=np.full(3, -1.0, np.float32), bmax=np.full(3, 1.0, np.float32), tau=np.float32(3 * spacing), spacing=spacing,
                radius=0.5, poses=poses, intrinsics=intrinsics, depth=depth, color=color, H=HW, W=HW)


def fuse(fx, dtype=np.float32, color=True, weight=None, trace=None):
    """the accumulators (acc_d, acc_w, acc_c) of a fixture's views, from zero"""
    n = fx["R"] ** 3
    acc_d, acc_w = np.zeros(n, dtype), np.zeros(n, dtype)
    acc_c = np.zeros((n, 3), dtype) if color else None
    integrate(acc_d, acc_w, acc_c, fx["depth"], fx["color"] if color else None, weight, fx["poses"], fx["intrinsics"], fx["R"], fx["bmin"],
              fx["bmax"], fx["tau"], dtype=dtype, trace=trace)
    return acc_d, acc_w, acc_c


def sign_changes(field, R):
    """Every lattice edge along an axis whose ends have different signs (<= 0 is inside): (crossing points [E,3] in lattice units by
    linear interpolation, E).  field [R,R,R]."""
    f = np.asarray(field, np.float64).reshape(R, R, R)
    idx = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), axis=-1).astype(np.float64)
    out = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, R - 1), slice(1, R)
        f0, f1 = f[tuple(lo)], f[tuple(hi)]
        cross = (f0 <= 0) != (f1 <= 0)
        t = f0[cross] / (f0[cross] - f1[cross])
        pts = idx[tuple(lo)][cross].copy()
        pts[:, a] += t
        out.append(pts)
    return np.concatenate(out)


# the hand-made views of the skip rules: a lattice of R = 3 over the box +-1 (its 27 points are exactly {-1, 0, 1}^3), images of H = 5
# rows and W = 7 columns, a camera with the identity rotation at (0, 0, -3) -- q = p + (0, 0, 3), q_z in {2, 3, 4}, r = q_z on the
# optical axis -- and fx = 7, fy = 5, cx = 3.5, cy = 2.5: at q_z = 2 the plane's corners project exactly onto x = 0 / 7 and y = 0 / 5.
HAND_R, HAND_H, HAND_W, HAND_TAU = 3, 5, 7, np.float32(0.5)
HAND_BMIN, HAND_BMAX = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)


def _hand_pose(o):
    M = np.eye(4, dtype=np.float32)
    M[:3, 3] = o
    return M


def hand_views():
    """name -> dict(pose [4,4], intrinsics [4], depth [H,W], weight [H,W], color [H,W,3]) -- all of the same 5 x 7 size, so that they
    also run merged in one call.  Where a rule is not about the weight, the weight is 1 everywhere."""
    H, W = HAND_H, HAND_W
    K = np.array([7, 5, 3.5, 2.5], np.float32)
    front = _hand_pose((0, 0, -3))
    ramp = (np.arange(H)[:, None] * W + np.arange(W)[None, :]).astype(np.float32)  # the flat pixel index j * W + i
    color = np.stack([3 * ramp, 3 * ramp + 1, 3 * ramp + 2], axis=-1)
    const = lambda v: np.full((H, W), v, np.float32)  # noqa: E731
    views = {}

    def add(name, pose=front, depth=np.inf, weight=1.0, K=K):
        views[name] = dict(pose=pose, intrinsics=K, depth=depth if isinstance(depth, np.ndarray) else const(depth),
                           weight=weight if isinstance(weight, np.ndarray) else const(weight), color=color)
    add("camera_inside", pose=_hand_pose((0, 0, 0)))  # q_z = p_z: only the plane p_z = 1 is in front of it
    add("readout", weight=1 + ramp)  # which pixel a voxel reads: acc_w = 1 + j * W + i, acc_c = acc_w * colour
    for name, d in (("depth_inf", np.inf), ("depth_nan", np.nan), ("depth_zero", 0.0), ("depth_negative", -1.0)):
        add(name, depth=d)
    centre = const(np.nan)  # only the pixel of the optical axis, (j, i) = (2, 3), holds a depth
    centre[2, 3] = 2.5  # the voxel (0, 0, 0) is at r = 3: s = -0.5 = -tau exactly
    add("s_at_minus_tau", depth=centre)
    below = centre.copy()
    below[2, 3] = np.nextafter(np.float32(2.5), np.float32(0))  # s = -0.5 - 2^-22: one float32 step of D below
    add("s_below_minus_tau", depth=below)
    for name, w in (("weight_zero", 0.0), ("weight_nan", np.nan), ("weight_negative", -1.0), ("weight_inf", np.inf)):
        add(name, weight=w)
    return views


def hand_view_1x1():
    """the 1 x 1 image: fx = fy = 1, cx = cy = 0.5, so x = p_x / q_z + 0.5 is exactly 0 / 1 at the corners of the plane q_z = 2"""
    return dict(pose=_hand_pose((0, 0, -3)), intrinsics=np.array([1, 1, 0.5, 0.5], np.float32), depth=np.full((1, 1), np.inf, np.float32),
                weight=np.full((1, 1), 2.0, np.float32), color=np.array([[[0.25, 0.5, 0.75]]], np.float32))


def stack_views(views):
    """(depth [V,H,W], color [V,H,W,3], weight [V,H,W], poses [V,4,4], intrinsics [V,4]) of a list of view dicts"""
    return (np.stack([v["depth"] for v in views]), np.stack([v["color"] for v in views]), np.stack([v["weight"] for v in views]),
            np.stack([v["pose"] for v in views]), np.stack([v["intrinsics"] for v in views]))
