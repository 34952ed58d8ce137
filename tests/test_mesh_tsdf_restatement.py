"""The depth-map fusion of csrc/pvd_hip_mesh_tsdf.h, checked on its numpy restatement (no GPU): the geometry it produces on an analytic
sphere, each skip rule on hand-made views whose outcome is known without running anything, the float32 restatement against its
float64 twin under a bound derived from the operation count, and the documented trade-off of unknown = +1."""
import numpy as np
import pytest

import mesh_tsdf_restatement as tr

U = 2.0 ** -24  # half an ulp of 1: the relative error of one float32 operation


@pytest.fixture(scope="module")
def sphere():
    fx = tr.sphere_fixture()  # R = 33, 64 x 64, 14 cameras at 3.2, tau = 3 spacings
    t32, t64 = [], []
    fx["acc32"] = tr.fuse(fx, np.float32, trace=t32)
    fx["acc64"] = tr.fuse(fx, np.float64, trace=t64)
    fx["trace32"], fx["trace64"] = t32, t64
    return fx


def _crossing_error(fx, field):
    """(number of sign changes along lattice edges, the largest |distance from the centre - radius| of one, in lattice spacings)"""
    pts = tr.sign_changes(field, fx["R"])
    rad = np.linalg.norm(pts * fx["spacing"] - 1.0, axis=1)
    return len(pts), float(np.abs(rad - fx["radius"]).max() / fx["spacing"])


def test_geometry_on_the_analytic_sphere(sphere):
    """Every sign change of the field along a lattice edge lies within ONE lattice spacing of the sphere, and there is no other sign
    change -- no inner shell where the unknown interior begins, no wall where a camera's view ends.  Measured with this restatement:
    0.443 spacings in float64 and in float32 (profiles/mesh_tsdf.txt)."""
    assert sphere["depth"].shape == (14, 64, 64) and sphere["R"] == 33 and abs(float(sphere["tau"]) - 3 * sphere["spacing"]) < 1e-7
    for dtype, acc in ((np.float64, sphere["acc64"]), (np.float32, sphere["acc32"])):
        field, totals = tr.finalize(acc[0], acc[1], 1.0, -1.0, dtype)
        count, worst = _crossing_error(sphere, field)
        print("sphere, %s: %d sign changes, the worst %.4f spacings from the sphere; totals %s" % (dtype.__name__, count, worst, totals))
        assert count > 1000  # the sphere's surface crosses about 4 pi (8 spacings)^2 * 1.5 lattice edges
        assert worst < 1.0
        assert totals[0] + totals[2] == 33 ** 3 and 0 < totals[1] < totals[0]
        # the centre is unknown (it is behind every camera's band) and, with unknown = -1, inside; the box's corners are outside
        f = field.reshape(33, 33, 33)
        assert f[16, 16, 16] == -1.0 and f[0, 0, 0] == 1.0 and f[32, 32, 32] == 1.0 and np.abs(field).max() <= 1.0


def test_unknown_plus_one_leaves_the_inner_shell(sphere):
    """The documented trade-off: with unknown = +1 the unseen interior counts as empty, and the band's far end, tau = 3 spacings behind
    the surface, becomes a second, inner shell.  Pinned so that nobody "fixes" it silently."""
    solid, _ = tr.finalize(sphere["acc32"][0], sphere["acc32"][1], 1.0, -1.0)
    empty, totals = tr.finalize(sphere["acc32"][0], sphere["acc32"][1], 1.0, 1.0)
    n_solid, _ = _crossing_error(sphere, solid)
    pts = tr.sign_changes(empty, sphere["R"])
    dev = (np.linalg.norm(pts * sphere["spacing"] - 1.0, axis=1) - sphere["radius"]) / sphere["spacing"]
    outer, inner = np.abs(dev) < 1.0, dev < -2.0
    assert outer.sum() == n_solid and inner.sum() > 100 and (outer | inner).all()
    assert empty.reshape(33, 33, 33)[16, 16, 16] == 1.0 and totals[2] > 0


# --------------------------------------------------------------------------------------------------- the skip rules, one by one
def _one_view(view, color=True, weight=True):
    n = tr.HAND_R ** 3
    acc_d, acc_w, acc_c = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    depth, col, wgt, poses, intr = tr.stack_views([view])
    tr.integrate(acc_d, acc_w, acc_c if color else None, depth, col if color else None, wgt if weight else None, poses, intr, tr.HAND_R,
                 tr.HAND_BMIN, tr.HAND_BMAX, tr.HAND_TAU)
    cube = (tr.HAND_R,) * 3
    return acc_d.reshape(cube), acc_w.reshape(cube), acc_c.reshape(cube + (3,))


def _in_view():
    """the voxels [i, j, k] (p = index - 1) the front camera sees: all but those of the plane p_z = -1 (q_z = 2) with p_x = 1 (x = 7
    = W exactly) or p_y = 1 (y = 5 = H exactly); p_x = -1 and p_y = -1 there land exactly on x = 0 and y = 0 and are kept"""
    seen = np.ones((3, 3, 3), bool)
    seen[2, :, 0] = False
    seen[:, 2, 0] = False
    return seen


VIEWS = tr.hand_views()


def test_the_lattice_of_the_hand_made_cases_is_exact():
    p = tr.lattice(3, tr.HAND_BMIN, tr.HAND_BMAX)
    assert p.dtype == np.float32 and p.shape == (27, 3)
    assert np.array_equal(p[13], [0, 0, 0]) and np.array_equal(p[0], [-1, -1, -1]) and np.array_equal(p[5], [-1, 0, 1])  # z fastest


def test_a_camera_inside_the_box_skips_what_is_beside_and_behind_it():
    acc_d, acc_w, _ = _one_view(VIEWS["camera_inside"])
    # q_z = p_z: the planes p_z = -1 (behind) and p_z = 0 (q_z == 0, the camera's own voxel among them) are skipped.  Of the plane
    # p_z = 1, x = 7 p_x + 3.5 and y = 5 p_y + 2.5: p_x = 1 gives 10.5 >= W, p_x = -1 gives -3.5 < 0, p_y = 1 gives 7.5 >= H and
    # p_y = -1 gives -2.5 < 0: the voxel on the optical axis is the only one in the image
    want = np.zeros((3, 3, 3), np.float32)
    want[1, 1, 2] = 1
    assert np.array_equal(acc_w, want) and np.array_equal(acc_d, want)


def test_the_image_borders_are_half_open():
    acc_d, acc_w, _ = _one_view(VIEWS["depth_inf"])
    assert np.array_equal(acc_w > 0, _in_view())
    assert np.array_equal(acc_d, acc_w) and set(np.unique(acc_w)) == {0.0, 1.0}  # free space: t = 1, w = 1


def test_the_pixel_a_voxel_reads_rows_and_columns_not_swapped():
    """weight[j][i] = 1 + j * 7 + i and colour[j][i][c] = 3 (j * 7 + i) + c on a 7 x 5 image: the sums name the pixel."""
    acc_d, acc_w, acc_c = _one_view(VIEWS["readout"])
    col = {2: [0, 3, None], 3: [1, 3, 5], 4: [1, 3, 5]}  # q_z -> i of p_x = -1, 0, 1: floor(7 p_x / q_z + 3.5)
    row = {2: [0, 2, None], 3: [0, 2, 4], 4: [1, 2, 3]}  # q_z -> j of p_y = -1, 0, 1: floor(5 p_y / q_z + 2.5)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                i, j = col[c + 2][a], row[c + 2][b]
                if i is None or j is None:
                    assert acc_w[a, b, c] == 0 and not acc_c[a, b, c].any()
                    continue
                flat = j * 7 + i
                assert acc_w[a, b, c] == 1 + flat and acc_d[a, b, c] == 1 + flat, (a, b, c)
                assert np.array_equal(acc_c[a, b, c], [(1 + flat) * (3 * flat + ch) for ch in range(3)]), (a, b, c)


@pytest.mark.parametrize("name", ["depth_nan", "depth_zero", "depth_negative", "weight_zero", "weight_nan", "weight_negative", "weight_inf"])
def test_no_observation_leaves_the_accumulators_alone(name):
    acc_d, acc_w, acc_c = _one_view(VIEWS[name])
    assert not acc_d.any() and not acc_w.any() and not acc_c.any()


def test_a_weight_is_ignored_when_none_is_passed():
    acc_d, acc_w, _ = _one_view(VIEWS["weight_zero"], weight=False)
    assert np.array_equal(acc_w > 0, _in_view())


def test_the_truncation_test_keeps_s_equal_to_minus_tau_and_drops_the_next_float():
    """Along the optical axis r = 2, 3, 4 exactly and only the axis' pixel holds a depth.  D = 2.5, tau = 0.5: s = 0.5 (t = 1), -0.5
    (t = -1, kept), -1.5 (dropped).  One float32 step less in D: s = -0.5 - 2^-22 < -tau, dropped."""
    for name, middle, near in (("s_at_minus_tau", 1.0, 1.0), ("s_below_minus_tau", 0.0, 1.0 - 2.0 ** -21)):
        acc_d, acc_w, _ = _one_view(VIEWS[name])
        want_w = np.zeros((3, 3, 3), np.float32)
        want_w[1, 1, 0], want_w[1, 1, 1] = 1, middle
        want_d = np.zeros((3, 3, 3), np.float32)
        want_d[1, 1, 0], want_d[1, 1, 1] = near, -middle  # the near voxel: s = D - 2 = 0.5 or 0.5 - 2^-22, t = s / 0.5
        assert np.array_equal(acc_w, want_w) and np.array_equal(acc_d, want_d), name


def test_a_one_by_one_image():
    v = tr.hand_view_1x1()
    acc_d, acc_w, acc_c = _one_view(v)
    # x = p_x / q_z + 0.5: exactly 0 (kept) and exactly 1 = W (skipped) at q_z = 2, inside (0, 1) behind it; the same in y
    assert np.array_equal(acc_w, np.where(_in_view(), np.float32(2), np.float32(0)))
    assert np.array_equal(acc_d, acc_w) and np.array_equal(acc_c[0, 0, 0], [0.5, 1.0, 1.5])


def test_batches_leave_the_bits_of_one_call():
    views = list(VIEWS.values())
    one = [np.zeros(27, np.float32), np.zeros(27, np.float32), np.zeros((27, 3), np.float32)]
    tr.integrate(*one, *tr.stack_views(views), 3, tr.HAND_BMIN, tr.HAND_BMAX, tr.HAND_TAU)
    many = [np.zeros(27, np.float32), np.zeros(27, np.float32), np.zeros((27, 3), np.float32)]
    for part in (views[:5], views[5:6], views[6:]):
        tr.integrate(*many, *tr.stack_views(part), 3, tr.HAND_BMIN, tr.HAND_BMAX, tr.HAND_TAU)
    for a, b in zip(one, many):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# --------------------------------------------------------------------------------------------------- float32 against float64
def rounding_bounds(fx, trace64, V):
    """What float32 rounding can do to a (voxel, view) pair, from the operation count (u = 2^-24 per operation; p, o, r are bounded by
    L = the largest |coordinate| + twice the largest extent for a lattice point -- three rounded operations -- and by r_max, the
    largest camera-to-voxel distance):
        d = p - o                       |err d_a| <= u (L + r)
        q_a: three products, two sums   |err q_a| <= sqrt(3) u (L + r) + 3 u r              =: e_q     (the rows of M are unit)
        x = (fx q_x) / q_z + cx         |err x|   <= (fx / q_z) (1 + |x - cx| / fx) e_q + 3 u |x - cx| + u |x|     =: e_x
        r = sqrt(sum of squares)        |err r|   <= sqrt(3) u (L + r) + 2.5 u r            =: e_r     (squares u, sums 2 u, halved, + u)
        s = D - r                       |err s|   <= e_r + u |s|                            =: e_s
        t = min(s / tau, 1)             |err t|   <= e_s / tau + u,  with |s| <= tau (1 + u) where t is not clipped to exactly 1
        acc_d: per view the product w t (u w) and one sum (u times the partial sum, at most sum w)
    -> |acc_d32 - acc_d64| <= u sum_w ((sqrt(3) (L + r_max) + 2.5 r_max) / tau + 3 + 2 V);  acc_w: V sums, u V sum_w (exact for w = 1)."""
    L = float(np.abs(np.concatenate([fx["bmin"], fx["bmax"]])).max() + 2 * (fx["bmax"] - fx["bmin"]).max())
    r_max = max(float(t["r"].max()) for t in trace64)
    tau = float(fx["tau"])
    e_q = np.sqrt(3) * U * (L + r_max) + 3 * U * r_max
    e_r = np.sqrt(3) * U * (L + r_max) + 2.5 * U * r_max
    per_weight = U * ((np.sqrt(3) * (L + r_max) + 2.5 * r_max) / tau + 3 + 2 * V)
    return e_q, e_r, per_weight


def fragile_pairs(fx, trace64, e_q, e_r):
    """[V, R^3] bool: the (voxel, view) pairs whose pixel choice or truncation test falls within rounding of its boundary"""
    out = []
    tau = float(fx["tau"])
    for t, K in zip(trace64, fx["intrinsics"].astype(np.float64)):
        with np.errstate(all="ignore"):
            front = t["qz"] > e_q
            e_x = (K[0] / t["qz"]) * (1 + np.abs(t["x"] - K[2]) / K[0]) * e_q + 3 * U * np.abs(t["x"] - K[2]) + U * np.abs(t["x"])
            e_y = (K[1] / t["qz"]) * (1 + np.abs(t["y"] - K[3]) / K[1]) * e_q + 3 * U * np.abs(t["y"] - K[3]) + U * np.abs(t["y"])
            near = np.abs(t["qz"]) <= e_q
            near |= front & ((np.abs(t["x"] - np.rint(t["x"])) <= e_x) | (np.abs(t["y"] - np.rint(t["y"])) <= e_y))
            near |= t["has_depth"] & np.isfinite(t["s"]) & (np.abs(t["s"] + tau) <= e_r + U * np.abs(t["s"]))
        out.append(near)
    return np.stack(out)


FRAGILE_CAP = 0.01


def test_float32_against_the_float64_twin(sphere):
    """The float32 restatement stays within the derived bound of its float64 twin on every voxel none of whose views is fragile; the
    fragile pairs are at most 1 % of all pairs (asserted), and outside them the two make the same decisions."""
    V, n = 14, 33 ** 3
    e_q, e_r, per_weight = rounding_bounds(sphere, sphere["trace64"], V)
    fragile = fragile_pairs(sphere, sphere["trace64"], e_q, e_r)
    share = fragile.mean()
    kept32 = np.stack([t["kept"] for t in sphere["trace32"]])
    kept64 = np.stack([t["kept"] for t in sphere["trace64"]])
    print("fragile pairs: %d of %d (%.4f %%); decisions that differ: %d" % (fragile.sum(), fragile.size, 100 * share, (kept32 != kept64).sum()))
    assert share <= FRAGILE_CAP
    assert not ((kept32 != kept64) & ~fragile).any()
    solid = ~fragile.any(axis=0)
    d32, w32, c32 = sphere["acc32"]
    d64, w64, c64 = sphere["acc64"]
    assert np.array_equal(w32[solid].astype(np.float64), w64[solid])  # w = 1: sums of small integers
    err = np.abs(d32.astype(np.float64) - d64)[solid]
    bound = per_weight * w64[solid]
    print("acc_d: the largest |float32 - float64| %.3e, bound %.3e per unit of weight (%.1f u)" % (err.max(), per_weight, per_weight / U))
    assert (err <= bound).all()
    # colour: per view one product and one sum on numbers of [0, 1] and w = 1: 2 u per view and unit of weight
    errc = np.abs(c32.astype(np.float64) - c64)[solid]
    assert (errc <= 2 * V * U * w64[solid][:, None]).all()


def test_sample_color_blends_only_what_was_observed(sphere):
    d32, w32, c32 = sphere["acc32"]
    R, lo, hi = 33, sphere["bmin"], sphere["bmax"]
    p = tr.lattice(R, lo, hi)
    seen = np.flatnonzero(w32 >= 1)
    got = tr.sample_color(c32, w32, R, lo, hi, 1.0, p[seen[:50]])
    want = np.clip(c32[seen[:50]] / w32[seen[:50], None], 0, 1)
    assert np.abs(got - want).max() <= 1e-5  # a lattice point: the blend of one corner (the others carry a weight of rounding size)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1.5, 0, 0], [0, 0, -1.001], [0, 0, 0]], np.float32)
    out = tr.sample_color(c32, w32, R, lo, hi, 1.0, bad)
    assert not out.any()  # not finite, outside, and the centre, none of whose corners is observed
    face = tr.sample_color(c32, w32, R, lo, hi, 1.0, np.array([[1, 1, 1], [-1, -1, -1], [1, 0.3, -0.2]], np.float32))
    assert np.isfinite(face).all() and (face >= 0).all() and (face <= 1).all() and face.any(axis=1).all()
    # min_weight above every count: nothing is observed
    assert not tr.sample_color(c32, w32, R, lo, hi, 15.0, p[seen[:50]]).any()


def test_sample_color_with_exactly_one_observed_corner(sphere):
    """A cell with ONE observed corner: the blend is m c / m of that corner, whatever its trilinear weight m -- also where m is 1e-9 or
    2^-60, next to the opposite corner -- and 0 exactly on the opposite corner, where m is 0.  One product and one quotient: 2 u."""
    case = tr.single_corner_case()
    corners = tr.observed_corners(case["acc_w"], case["R"], 1.0)
    assert corners.sum() == 8 and (corners[1:3, 1:3, 1:3] == 1).all()
    got = tr.sample_color(case["acc_c"], case["acc_w"], case["R"], case["bmin"], case["bmax"], 1.0, case["points"])
    zero = case["exact_zero"]
    assert zero.sum() == 8 and not got[zero].any()
    want = case["color"].astype(np.float64)
    assert (np.abs(got[~zero].astype(np.float64) - want) <= 2.5 * U * want).all()
    # and on the sphere: the cells at the rim of the unobserved ball that have exactly one observed corner
    d32, w32, c32 = sphere["acc32"]
    count = tr.observed_corners(w32, 33, 1.0)
    cells = np.argwhere(count == 1)
    assert len(cells) > 0
    pts = (-1.0 + (cells + np.array([0.3, 0.6, 0.45])) * sphere["spacing"]).astype(np.float32)
    got = tr.sample_color(c32, w32, 33, sphere["bmin"], sphere["bmax"], 1.0, pts)
    seen = (w32 >= 1).reshape(33, 33, 33)
    for row, cell in zip(got, cells):
        (corner,) = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1) if seen[cell[0] + a, cell[1] + b, cell[2] + c]]
        n = ((cell[0] + corner[0]) * 33 + cell[1] + corner[1]) * 33 + cell[2] + corner[2]
        want = np.clip(c32[n].astype(np.float64) / w32[n], 0, 1)
        assert (np.abs(row - want) <= 4 * U * np.maximum(want, 1e-3)).all(), cell
