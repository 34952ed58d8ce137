"""numpy restatement of aaai2023-pvd_amd/csrc/pvd_hip_mesh_project.h: pvd_mesh_project_integrate and pvd_mesh_project_finalize,
operation for operation in the order the header writes them (not from the kernel).  Every array and scalar of steps 1 .. 7 and 9 is of
ONE dtype, so nothing is promoted: dtype=np.float32 is the restatement the kernels are compared with bit for bit, dtype=np.float64 its
twin -- the same decisions in the same order on the same float32 inputs -- the reference of the rounding bound.  numpy rounds every
elementwise operation on its own and fuses nothing; its division and square root are correctly rounded.

Step 8, the occlusion, is brute force: every ray that reaches it against every triangle, no grid -- which is what "independent of G and
the box" is measured against.  Steps 1 and 2 of hit() are mesh_ray_restatement._ray_constants, by import; steps 3 .. 7 are restated
here because mesh_ray_restatement.hit_matrix takes float32 directions and this ray's direction D = (double)o - (double)o' is a float64
difference.  For the same reason the edge-on measure is mesh_expose_restatement.det_ratio's formula evaluated on that float64 ray (and
it is checked against det_ratio itself on rays whose direction is exact in float32).

Also here, because the CPU tests and the GPU tests share them: the hand-made views of the skip rules, the patterned sphere and the
quad over a plane."""
import functools

import numpy as np

import mesh_dist_restatement as md
import mesh_expose_restatement as xr
import mesh_ray_restatement as rr
import mesh_tsdf_restatement as tr

F64 = np.float64
MAX_SIDE = 16384
MAX_POWER = 8
SIDES = ("front", "both")
MODES = ("blend", "best")
TOTALS = ("seen", "unseen")
DET_BOUND = xr.DET_BOUND


# ------------------------------------------------------------------------------------------------------------------ step 8
def blocked(start, camera, vertices, triangles, block=64):
    """(bool [n], the smallest det ratio): is the ray from start [n,3] f32 (t = 0) to camera [n,3] f32 (t = 1) hit by some valid triangle
    with 0 <= t < 1; the ratio is |det| / L^2 (mesh_expose_restatement.det_ratio) over every (ray, triangle) pair that steps 5 and 6 do
    not miss -- inf without one.  A ray with a number that is not finite or with D = 0 is blocked by nothing."""
    s32, c32 = np.asarray(start, np.float32).reshape(-1, 3), np.asarray(camera, np.float32).reshape(-1, 3)
    n = len(s32)
    out, smallest = np.zeros(n, bool), np.inf
    tv, tt = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    idx = np.nonzero(md.valid_triangles(tv, tt))[0] if len(tt) else np.zeros(0, np.int64)
    o_all = s32.astype(F64)
    d_all = c32.astype(F64) - o_all
    ok = np.all(np.isfinite(s32), axis=1) & np.all(np.isfinite(c32), axis=1) & np.any(d_all != 0, axis=1)
    rays = np.nonzero(ok)[0]
    if not len(idx) or not len(rays):
        return out, smallest
    corners = tv[tt[idx]].astype(F64)  # [T',3 corners,3 axes]
    with np.errstate(all="ignore"):
        for b in range(0, len(rays), block):
            r = rays[b:b + block]
            o, d = o_all[r], d_all[r]
            kx, ky, kz, Sx, Sy, Sz = rr._ray_constants(o, d)
            P = corners[None, :, :, :] - o[:, None, None, :]  # [m,T',3,3]
            m = len(r)

            def axis(k):
                return np.take_along_axis(P, np.broadcast_to(k[:, None, None, None], (m, P.shape[1], 3, 1)), axis=3)[..., 0]
            Px, Py, Pz = axis(kx), axis(ky), axis(kz)
            X = Px - Sx[:, None, None] * Pz
            Y = Py - Sy[:, None, None] * Pz
            Z = Sz[:, None, None] * Pz
            U = X[..., 2] * Y[..., 1] - Y[..., 2] * X[..., 1]
            V = X[..., 0] * Y[..., 2] - Y[..., 0] * X[..., 2]
            W = X[..., 1] * Y[..., 0] - Y[..., 1] * X[..., 0]
            miss = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
            det = (U + V) + W
            miss |= det == 0
            t = ((U * Z[..., 0] + V * Z[..., 1]) + W * Z[..., 2]) / det
            out[r] = np.any(~miss & (t >= 0) & (t < 1), axis=1)
            if (~miss).any():
                L = np.abs(P).max(axis=(2, 3))
                smallest = min(smallest, float((np.abs(det) / (L * L))[~miss].min()))
    return out, smallest


# ------------------------------------------------------------------------------------------------------------------ integrate
def integrate(acc_c, acc_w, points, normals, color, weight, poses, intrinsics, vertices, triangles, cos_min=0.0, power=0, bias=0.0,
              sides="front", mode="blend", dtype=np.float32, trace=None):
    """acc_c [N,3] and acc_w [N] (arrays of `dtype`, changed in place) <- steps 1 .. 9 for points, normals [N,3], color [V,H,W,3],
    weight [V,H,W] or None, poses [V,4,4], intrinsics [V,4] (float32 arrays) and the mesh.  Returns the smallest det ratio over the
    pairs step 8 tested.  trace: a list that receives, per view, dict(c, x, y, qz, w, facing, in_front, in_frame, finite, weighted,
    kept) over all points (numbers are garbage where an earlier step already skipped the point; the masks are those after steps 2, 3,
    4, 6 (colour), 6 (weight) and 8)."""
    assert sides in SIDES and mode in MODES and 0 <= int(power) <= MAX_POWER
    V, H, W = color.shape[:3]
    assert 2 <= H <= MAX_SIDE and 2 <= W <= MAX_SIDE
    p32, n32 = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    p, nr = p32.astype(dtype), n32.astype(dtype)
    zero, half, one = dtype(0), dtype(0.5), dtype(1)
    cos_min, bias = dtype(np.float32(cos_min)), dtype(np.float32(bias))
    smallest = np.inf
    with np.errstate(all="ignore"):
        L = np.sqrt((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2])
        part = np.all(np.isfinite(p32), axis=1) & np.all(np.isfinite(n32), axis=1) & (L > zero) & (L < dtype(np.inf))
        u = nr / L[:, None]
        x_hi, y_hi = dtype(W) - half, dtype(H) - half
        for v in range(V):
            M = poses[v].astype(np.float32).astype(dtype)
            fx, fy, cx, cy = intrinsics[v].astype(np.float32).astype(dtype)
            o = M[:3, 3]
            # 1
            ex, ey, ez = o[0] - p[:, 0], o[1] - p[:, 1], o[2] - p[:, 2]
            r = np.sqrt((ex * ex + ey * ey) + ez * ez)
            keep = part & (r > zero)
            # 2
            c = ((u[:, 0] * ex + u[:, 1] * ey) + u[:, 2] * ez) / r
            s = np.ones_like(c)
            if sides == "both":
                s = np.where(c < zero, -one, one).astype(dtype)
                c = np.abs(c)
            keep &= c > cos_min
            facing = keep.copy()
            # 3
            dx, dy, dz = p[:, 0] - o[0], p[:, 1] - o[1], p[:, 2] - o[2]
            qx = (M[0, 0] * dx + M[1, 0] * dy) + M[2, 0] * dz
            qy = (M[0, 1] * dx + M[1, 1] * dy) + M[2, 1] * dz
            qz = (M[0, 2] * dx + M[1, 2] * dy) + M[2, 2] * dz
            keep &= qz > zero
            in_front = keep.copy()
            x = (fx * qx) / qz + cx
            y = (fy * qy) / qz + cy
            # 4
            keep &= (x >= half) & (x <= x_hi) & (y >= half) & (y <= y_hi)
            in_frame = keep.copy()
            # 5
            a, b = x - half, y - half
            i = np.minimum(np.where(keep, np.floor(a), zero).astype(np.int64), W - 2)
            j = np.minimum(np.where(keep, np.floor(b), zero).astype(np.int64), H - 2)
            f, g = a - i.astype(dtype), b - j.astype(dtype)
            # 6
            f1, g1 = one - f, one - g
            m00, m10, m01, m11 = f1 * g1, f * g1, f1 * g, f * g
            img = color[v]
            I00, I10, I01, I11 = (img[j + db, i + da].astype(dtype) for da, db in ((0, 0), (1, 0), (0, 1), (1, 1)))
            keep &= np.all(np.isfinite(I00), axis=1) & np.all(np.isfinite(I10), axis=1) & np.all(np.isfinite(I01), axis=1) \
                & np.all(np.isfinite(I11), axis=1)
            finite = keep.copy()
            C = ((m00[:, None] * I00 + m10[:, None] * I10) + m01[:, None] * I01) + m11[:, None] * I11
            # 7
            w = np.ones_like(c)
            for _ in range(int(power)):
                w = w * c
            if weight is not None:
                wi = weight[v]
                w00, w10, w01, w11 = (wi[j + db, i + da].astype(dtype) for da, db in ((0, 0), (1, 0), (0, 1), (1, 1)))
                wp = ((m00 * w00 + m10 * w10) + m01 * w01) + m11 * w11
                keep &= (wp > zero) & (wp < dtype(np.inf))
                w = w * wp
            weighted = keep.copy()
            # 8: float32 start in the float32 restatement; the twin keeps its own
            start = p + (s * bias)[:, None] * u
            rows = np.nonzero(keep)[0]
            if len(rows):
                hit, ratio = blocked(start[rows].astype(np.float32) if dtype == np.float32 else _f32_like(start[rows]),
                                     np.broadcast_to(poses[v].astype(np.float32)[:3, 3], (len(rows), 3)), vertices, triangles)
                smallest = min(smallest, ratio)
                keep[rows[hit]] = False
            # 9
            if mode == "best":
                take = keep & (w > acc_w)
                acc_w[take] = w[take]
                acc_c[take] = C[take]
            else:
                acc_w[keep] = (acc_w + w)[keep]
                acc_c[keep] = (acc_c + w[:, None] * C)[keep]
            if trace is not None:
                trace.append(dict(c=c, x=x, y=y, qz=qz, w=w, facing=facing, in_front=in_front, in_frame=in_frame, finite=finite,
                                  weighted=weighted, kept=keep.copy()))
    return smallest


def _f32_like(a):
    """The float64 twin's ray start, rounded to float32 once: blocked() takes float32 starts (the twin's occlusion decision is that of
    a start within one rounding of its own)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, F64).astype(np.float32)


def project(points, normals, color, weight, poses, intrinsics, vertices, triangles, dtype=np.float32, trace=None, **kw):
    """(acc_c, acc_w, smallest det ratio) from zeroed accumulators"""
    N = np.asarray(points).reshape(-1, 3).shape[0]
    acc_c, acc_w = np.zeros((N, 3), dtype), np.zeros(N, dtype)
    ratio = integrate(acc_c, acc_w, points, normals, color, weight, poses, intrinsics, vertices, triangles, dtype=dtype, trace=trace, **kw)
    return acc_c, acc_w, ratio


def finalize(acc_c, acc_w, min_weight, mode, fallback, dtype=np.float32):
    """(colors [N,3], seen [N] uint8, totals (seen, unseen)); fallback [N,3]: what the caller filled colors with."""
    assert mode in MODES
    with np.errstate(all="ignore"):
        seen = acc_w >= dtype(np.float32(min_weight))
        q = acc_c if mode == "best" else acc_c / acc_w[:, None]
        col = np.fmin(np.fmax(q, dtype(0)), dtype(1))  # fmaxf / fminf: a NaN gives the other operand
    colors = np.where(seen[:, None], col, np.asarray(fallback, np.float32).astype(dtype)).astype(dtype)
    return colors, seen.astype(np.uint8), (int(seen.sum()), int((~seen).sum()))


# --------------------------------------------------------------------------------------------------------- the hand-made cases
# One camera with the identity rotation at (0, 0, -3) that looks along +z, images of H = 5 rows and W = 7 columns, fx = fy = 4,
# cx = 3.5, cy = 2.5.  The points lie in the plane z = -1, so q_z = 2 and x = 2 p_x + 3.5, y = 2 p_y + 2.5 without rounding: the frame
# 0.5 <= x <= 6.5, 0.5 <= y <= 4.5 is exactly |p_x| <= 1.5, |p_y| <= 1.  The colour of pixel (i, j) is ((k, k + 35, k + 70) / 128 with
# k = j * W + i: every value and every bilinear mix at quarter positions is exact in float32.
HAND_H, HAND_W = 5, 7
HAND_K = np.array([4, 4, 3.5, 2.5], np.float32)
# the mesh of the hand-made cases: 0 a blocker in the plane z = -2, between the camera and the point (1, 0.5, -1) only; 1 a large
# triangle BEHIND the camera (z = -4), which every ray's line meets at t = 1.5; 2 a small one in the plane z = -1.25 over the point
# (-1, -0.5, -1), 0.25 above it and so below a start lifted by bias = 0.5; 3 an invalid one (a NaN corner) across the optical axis
HAND_VERTICES = np.array([(0.25, 0.125, -2), (1, 0.125, -2), (0.25, 1, -2),
                          (-1, -1, -4), (3, -1, -4), (-1, 3, -4),
                          (-1, -0.5, -1.25), (-0.75, -0.5, -1.25), (-1, -0.25, -1.25),
                          (-1, -1, -2), (3, -1, -2), (np.nan, 3, -2)], np.float32)
HAND_TRIANGLES = np.arange(12, dtype=np.int32).reshape(4, 3)


def _hand_pose(o=(0, 0, -3)):
    M = np.eye(4, dtype=np.float32)
    M[:3, 3] = o
    return M


def hand_ramp():
    return (np.arange(HAND_H)[:, None] * HAND_W + np.arange(HAND_W)[None, :]).astype(np.float32)


def hand_color(k):
    """the colour of the (fractional) ramp value k"""
    k = np.float32(k)
    return np.array([k, k + np.float32(35), k + np.float32(70)], np.float32) / np.float32(128)


def hand_views():
    """name -> dict(pose [4,4], intrinsics [4], color [H,W,3], weight [H,W]) -- all of the same size and camera, so that they also run
    merged in one call: the plain ramp, a NaN and an infinite colour value next to the optical axis, and the weights 0, inf, NaN and 2."""
    ramp = hand_ramp()
    color = np.stack([ramp, ramp + 35, ramp + 70], axis=-1).astype(np.float32) / np.float32(128)
    views = {}

    def add(name, color=color, weight=1.0):
        views[name] = dict(pose=_hand_pose(), intrinsics=HAND_K, color=color, weight=np.full((HAND_H, HAND_W), weight, np.float32))
    add("ramp")
    bad = color.copy()
    bad[2, 4, 1] = np.nan  # pixel (i, j) = (4, 2): the right neighbour of the optical axis' pixel
    add("nan_pixel", color=bad)
    bad = color.copy()
    bad[3, 3, 2] = np.inf  # the lower neighbour
    add("inf_pixel", color=bad)
    for name, w in (("weight_zero", 0.0), ("weight_inf", np.inf), ("weight_nan", np.nan), ("weight_two", 2.0)):
        add(name, weight=w)
    return views


AXIS, OFF = (0.0, 0.0, -1.0), (0.25, 0.125, -1.0)  # the optical axis' point (pixel (3, 2), f = g = 0) and one with f = 0.5, g = 0.25
TOWARDS = (0.0, 0.0, -2.0)  # a normal that faces the camera, not of unit length
TILTED = (0.0, 3.0, -4.0)  # L = 5; from the axis point c = (float32)0.8


def hand_cases():
    """name -> dict(point, normal, view, weighted, kw, acc_w, ramp): ONE point against ONE view of hand_views() over the hand-made mesh
    with the keywords kw of integrate (cos_min, power, bias, sides); weighted: the view's weight image is passed.  Expected: acc_w, and
    where it is not 0 the ramp value whose colour times acc_w is acc_c -- all written out by hand."""
    c08 = np.float32(0.8)
    cases = {}

    def add(name, point, normal=TOWARDS, view="ramp", weighted=False, acc_w=0.0, ramp=None, **kw):
        cases[name] = dict(point=np.array(point, np.float32), normal=np.array(normal, np.float32), view=view, weighted=weighted, kw=kw,
                           acc_w=np.float32(acc_w), ramp=ramp)
    add("on_axis", AXIS, acc_w=1, ramp=17)  # pixel (3, 2): k = 2 * 7 + 3; the triangle behind the camera (t = 1.5) does not block
    add("bilinear", OFF, acc_w=1, ramp=19.25)  # 17 + 0.5 * 1 + 0.25 * 7
    add("behind_the_camera", (0, 0, -4), normal=(0, 0, 1))  # faces the camera (c = 1) but q_z = -1
    for name, pt in (("out_left", (-1.75, 0, -1)), ("out_right", (1.75, 0, -1)), ("out_top", (0, -1.25, -1)), ("out_bottom", (0, 1.25, -1)),
                     ("just_out_right", (1.5 + 2.0 ** -21, 0, -1)),  # x = 6.5 + 2^-20, two float32 steps past the border, exactly
                     ("just_out_top", (0, -1 - 2.0 ** -21, -1))):  # y = 0.5 - 2^-20
        add(name, pt)
    # exactly on the border x = 0.5 / 6.5, y = 0.5 / 4.5: kept, and the clamp i = W - 2 with f = 1 reads the last column
    add("border_left", (-1.5, 0, -1), acc_w=1, ramp=14)  # pixel (0, 2)
    add("border_right", (1.5, 0, -1), acc_w=1, ramp=20)  # pixel (6, 2) through i = 5, f = 1
    add("border_top", (0, -1, -1), acc_w=1, ramp=3)  # pixel (3, 0)
    add("border_bottom", (0, 1, -1), acc_w=1, ramp=31)  # pixel (3, 4) through j = 3, g = 1
    add("border_corner", (1.5, 1, -1), acc_w=1, ramp=34)  # pixel (6, 4): m11 = 1
    # facing: u = (0, 0.6, -0.8), e = (0, 0, -2), r = 2: c = ((0 + 0) + 1.6) / 2 = (float32)0.8
    add("cosine_squared", AXIS, normal=TILTED, power=2, acc_w=c08 * c08, ramp=17)
    add("cosine_to_the_eighth", AXIS, normal=TILTED, power=8, acc_w=((((((c08 * c08) * c08) * c08) * c08) * c08) * c08) * c08, ramp=17)
    add("c_equals_cos_min", AXIS, normal=TILTED, cos_min=c08)
    add("c_just_above_cos_min", AXIS, normal=TILTED, cos_min=np.nextafter(c08, np.float32(0)), acc_w=1, ramp=17)
    add("back_facing_front", AXIS, normal=(0, 0, 2))  # c = -1
    add("back_facing_both", AXIS, normal=(0, 0, 2), sides="both", acc_w=1, ramp=17)  # s = -1, c = 1
    add("blocked", (1, 0.5, -1))  # the line to the camera crosses z = -2 at (0.5, 0.25), inside triangle 0, at t = 0.5
    # x = 2 * -1 + 3.5 = 1.5, y = 2 * -0.5 + 2.5 = 1.5: pixel (1, 1), k = 8; the start (-1, -0.5, -1.5) is past triangle 2 (t = -1 / 6)
    add("blocker_behind_the_start", (-1, -0.5, -1), bias=0.5, acc_w=1, ramp=8)
    add("blocker_in_front_of_the_start", (-1, -0.5, -1))  # bias = 0: triangle 2 is hit at t = 0.125
    add("nan_pixel", OFF, view="nan_pixel")
    add("nan_pixel_with_weight_zero_on_it", AXIS, view="nan_pixel")  # m10 = 0, and the view is skipped all the same
    add("inf_pixel", OFF, view="inf_pixel")
    add("weight_zero", OFF, view="weight_zero", weighted=True)
    add("weight_inf", OFF, view="weight_inf", weighted=True)
    add("weight_nan", OFF, view="weight_nan", weighted=True)
    add("weight_two", OFF, view="weight_two", weighted=True, acc_w=2, ramp=19.25)
    add("weight_ignored_when_not_passed", OFF, view="weight_zero", acc_w=1, ramp=19.25)
    add("nan_point", (np.nan, 0, -1))
    add("inf_normal", AXIS, normal=(0, np.inf, -1))
    add("zero_normal", AXIS, normal=(0, 0, 0))
    add("camera_at_the_point", (0, 0, -3))  # r = 0
    return cases


def hand_stack(names=None):
    """(color [V,H,W,3], weight [V,H,W], poses [V,4,4], intrinsics [V,4]) of the named views (default: all, in hand_views' order)"""
    views = hand_views()
    vs = [views[k] for k in (names or list(views))]
    return (np.stack([v["color"] for v in vs]), np.stack([v["weight"] for v in vs]), np.stack([v["pose"] for v in vs]),
            np.stack([v["intrinsics"] for v in vs]))


def hand_points():
    """(points, normals): every point and normal of hand_cases(), in order -- for the run of all of them against all views in one call"""
    cs = hand_cases().values()
    return np.stack([c["point"] for c in cs]), np.stack([c["normal"] for c in cs])


# --------------------------------------------------------------------------------------------------------- the patterned sphere
PATTERN_K = 3.0  # the wave number of the pattern 0.5 + 0.5 sin(k x)
SPHERE_COS_MIN = 0.5


def pattern(x):
    """[...,3]: 0.5 + 0.5 sin(k x) per coordinate (float64)"""
    return 0.5 + 0.5 * np.sin(PATTERN_K * np.asarray(x, F64))


@functools.lru_cache(maxsize=None)
def sphere_mesh(R=9):
    """(vertices, triangles, unit normals [V,3] f32) of mesh_expose_restatement's "ball" (radius 0.95 about CENTRE), read-only; the
    normals point away from the centre."""
    v, t = xr.fixture("ball", R)
    n = v.astype(F64) - np.array(xr.CENTRE)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    n.setflags(write=False)
    return v, t, n


def camera_rays(pose, K, H, W):
    """(origins, directions) [H*W,3] f32 through the pixel centres, not normalised: M[:3,:3] ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1)"""
    M, K = pose.astype(F64), np.asarray(K, F64)
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([(ii - K[2]) / K[0], (jj - K[3]) / K[1], np.ones_like(ii)], axis=-1).reshape(-1, 3) @ M[:3, :3].T
    return np.broadcast_to(pose[:3, 3].astype(np.float32), d.shape).copy(), d.astype(np.float32)


def _first_hit_tiled(pose, K, H, W, o, d, vertices, triangles, tile=8):
    """(t [H*W] f32, hit [H*W] int32: 0 or -1) of mesh_ray_restatement.first_hit, a tile of pixels at a time against the triangles whose
    projected bounding box (a pixel wider on every side) meets the tile: first_hit is a dense [rays, triangles] evaluation, and a tile
    sees a few dozen of the mesh's triangles.  Only for a camera that has the whole mesh in front of it."""
    M, K = pose.astype(F64), np.asarray(K, F64)
    q = (vertices.astype(F64) - M[:3, 3]) @ M[:3, :3]
    assert (q[:, 2] > 0).all()
    px, py = K[0] * q[:, 0] / q[:, 2] + K[2], K[1] * q[:, 1] / q[:, 2] + K[3]
    tx, ty = px[triangles], py[triangles]
    x0, x1, y0, y1 = tx.min(axis=1) - 1, tx.max(axis=1) + 1, ty.min(axis=1) - 1, ty.max(axis=1) + 1
    t_out, hit = np.full(H * W, np.inf, np.float32), np.full(H * W, -1, np.int32)
    for j0 in range(0, H, tile):
        for i0 in range(0, W, tile):
            sel = np.nonzero((x1 >= i0) & (x0 <= i0 + tile) & (y1 >= j0) & (y0 <= j0 + tile))[0]
            if not len(sel):
                continue
            jj, ii = np.meshgrid(np.arange(j0, min(j0 + tile, H)), np.arange(i0, min(i0 + tile, W)), indexing="ij")
            rows = (jj * W + ii).ravel()
            th, tri, _ = rr.first_hit(o[rows], d[rows], vertices, triangles[sel])
            t_out[rows], hit[rows] = th, np.where(tri >= 0, 0, -1)
    return t_out, hit


@functools.lru_cache(maxsize=None)
def sphere_views(R=9, HW=64, n=14, distance=3.2):
    """dict(poses [n,4,4], intrinsics [n,4], color [n,HW,HW,3], weight [n,HW,HW], fx, distance): the images of the end-to-end case -- the
    restatement's sphere mesh first-hit cast (mesh_ray_restatement.first_hit) from mesh_tsdf_restatement.sphere_cameras, every pixel
    coloured pattern(hit point); pixels that miss the mesh are NaN with the weight 0.  The focal length lets the ball (radius 0.95 at
    the distance 3.2) fill most of the frame: tan(half the field of view) = 0.36."""
    v, t, _ = sphere_mesh(R)
    poses = tr.sphere_cameras(n, distance)
    fx = 0.5 * HW / 0.36
    K = np.array([fx, fx, HW / 2, HW / 2], np.float32)
    color = np.full((n, HW, HW, 3), np.nan, np.float32)
    weight = np.zeros((n, HW, HW), np.float32)
    for k, M in enumerate(poses):
        o, d = camera_rays(M, K, HW, HW)
        th, tri = _first_hit_tiled(M, K, HW, HW, o, d, v, t)
        hit = tri >= 0
        x = o.astype(F64) + th.astype(F64)[:, None] * d.astype(F64)
        color[k].reshape(-1, 3)[hit] = pattern(x[hit]).astype(np.float32)
        weight[k].reshape(-1)[hit] = 1.0
    out = dict(poses=poses, intrinsics=np.tile(K, (n, 1)), color=color, weight=weight, fx=float(fx), distance=float(distance))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def sphere_bound(fx, distance, radius=0.95, cos_min=SPHERE_COS_MIN):
    """0.5 k sqrt 2 (r / fx) / cos_min: the pattern's slope per coordinate is at most 0.5 k; a bilinear mix reads pixels at most one
    pixel diagonal (sqrt 2) from the projection; a pixel subtends r / fx at the distance r <= distance + radius; on a surface seen
    under the cosine c > cos_min that footprint is stretched by 1 / c."""
    return 0.5 * PATTERN_K * np.sqrt(2.0) * ((distance + radius) / fx) / cos_min


# --------------------------------------------------------------------------------------------------------- a quad over a plane
def occluder_case():
    """dict(vertices, triangles, points, normals, color, poses, intrinsics, shadowed [N] bool): the plane z = 0 (two large triangles)
    with a quad (two triangles) at z = 0.5 over |x|, |y| <= 0.5, one camera straight above at z = 4 whose image is a constant
    (0.25, 0.5, 0.75), and a lattice of points ON the plane with the normal +z.  A point is shadowed where the line to the camera
    crosses z = 0.5 inside the quad: |x|, |y| < 0.5 * 4 / 3.5; the lattice is chosen off that border."""
    vertices = np.array([(-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0), (-0.5, -0.5, 0.5), (0.5, -0.5, 0.5), (0.5, 0.5, 0.5), (-0.5, 0.5, 0.5)],
                        np.float32)
    triangles = np.array([(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)], np.int32)
    g = (np.arange(9) - 4) * 0.25 + 0.03
    X, Y = np.meshgrid(g, g, indexing="ij")
    points = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], axis=1).astype(np.float32)
    normals = np.tile(np.array([0, 0, 1], np.float32), (len(points), 1))
    M = np.eye(4, dtype=np.float32)  # looks along world -z from (0, 0, 4): the camera's z axis is (0, 0, -1), its y axis (0, -1, 0)
    M[:3, 1], M[:3, 2], M[:3, 3] = (0, -1, 0), (0, 0, -1), (0, 0, 4)
    HW = 16
    color = np.tile(np.array([0.25, 0.5, 0.75], np.float32), (1, HW, HW, 1))
    K = np.array([[HW, HW, HW / 2, HW / 2]], np.float32)  # tan(half) = 0.5: the frame covers |x|, |y| < 2 at the plane
    edge = 0.5 * 4 / 3.5
    shadowed = (np.abs(points[:, 0]) < edge) & (np.abs(points[:, 1]) < edge)
    assert (np.abs(np.abs(points[:, :2]) - edge) > 0.01).all()
    return dict(vertices=vertices, triangles=triangles, points=points, normals=normals, color=color, poses=M[None], intrinsics=K,
                shadowed=shadowed)
