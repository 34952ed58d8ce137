"""tests/mesh_project_restatement.py, the numpy restatement of csrc/pvd_hip_mesh_project.h that tests/test_hip_mesh_project.py compares
the kernels with, pinned first (no GPU): every skip rule on a hand-made case against values written out by hand, batches against one
call, ties in mode "best", the float32 restatement against its float64 twin under a bound derived from the operation count, the
patterned sphere end to end under the bound 0.5 k sqrt 2 (r / fx) / cos_min, and a quad that shadows part of a plane."""
import numpy as np
import pytest

import mesh_expose_restatement as xr
import mesh_project_restatement as pr

U = 2.0 ** -24
SPHERE_BIAS = np.float32(1e-3 * np.sqrt(3.0) * 2 * 0.95)  # 1e-3 of the box diagonal of a ball of radius 0.95


@pytest.fixture(scope="module")
def sphere():
    v, t, n = pr.sphere_mesh()
    sv = pr.sphere_views()
    kw = dict(cos_min=pr.SPHERE_COS_MIN, power=2, bias=SPHERE_BIAS)
    t32, t64 = [], []
    acc32 = pr.project(v, n, sv["color"], sv["weight"], sv["poses"], sv["intrinsics"], v, t, trace=t32, **kw)
    acc64 = pr.project(v, n, sv["color"], sv["weight"], sv["poses"], sv["intrinsics"], v, t, dtype=np.float64, trace=t64, **kw)
    return dict(v=v, t=t, n=n, sv=sv, kw=kw, acc32=acc32, acc64=acc64, t32=t32, t64=t64)


def _run_case(case, dtype=np.float32, prefill=None):
    view = pr.hand_views()[case["view"]]
    acc_c, acc_w = np.zeros((1, 3), dtype), np.zeros(1, dtype)
    if prefill is not None:
        acc_c[:] = prefill
        acc_w[:] = prefill
    pr.integrate(acc_c, acc_w, case["point"][None], case["normal"][None], view["color"][None], view["weight"][None] if case["weighted"] else None,
                 view["pose"][None], view["intrinsics"][None], pr.HAND_VERTICES, pr.HAND_TRIANGLES, dtype=dtype, **case["kw"])
    return acc_c[0], acc_w[0]


@pytest.mark.parametrize("name", list(pr.hand_cases()))
def test_a_hand_made_case_against_values_written_out_by_hand(name):
    case = pr.hand_cases()[name]
    acc_c, acc_w = _run_case(case)
    assert acc_w == case["acc_w"], (name, acc_w)
    want = np.zeros(3, np.float32) if case["ramp"] is None else case["acc_w"] * pr.hand_color(case["ramp"])
    assert np.array_equal(acc_c, want), (name, acc_c, want)
    if case["ramp"] is None:  # a skipped view leaves whatever the accumulators held
        acc_c, acc_w = _run_case(case, prefill=7.0)
        assert acc_w == 7.0 and (acc_c == 7.0).all(), name
        case = dict(case, kw=dict(case["kw"], mode="best"))
        acc_c, acc_w = _run_case(case, prefill=0.0)
        assert acc_w == 0.0 and (acc_c == 0.0).all(), name


def test_the_hand_made_cases_cover_every_skip_rule():
    names = set(pr.hand_cases())
    for rule in ("behind_the_camera", "out_left", "out_right", "out_top", "out_bottom", "border_left", "border_right", "border_top",
                 "border_bottom", "c_equals_cos_min", "back_facing_front", "back_facing_both", "blocked", "on_axis",
                 "blocker_behind_the_start", "nan_pixel", "inf_pixel", "weight_zero", "weight_inf", "nan_point", "zero_normal"):
        assert rule in names, rule
    # the quantities the comments of the cases state: the ray of "blocked" meets triangle 0 at t = 0.5, every ray's line meets the
    # triangle behind the camera at t = 1.5 only, and the lifted start of "blocker_behind_the_start" is past triangle 2
    cam = np.array([[0, 0, -3]], np.float32)
    one = lambda k: (pr.HAND_VERTICES, pr.HAND_TRIANGLES[k:k + 1])  # noqa: E731
    assert pr.blocked(np.array([[1, 0.5, -1]], np.float32), cam, *one(0))[0][0]
    assert not pr.blocked(np.array([[0, 0, -1]], np.float32), cam, *one(1))[0][0]
    assert pr.blocked(np.array([[0, 0, -1]], np.float32), np.array([[0, 0, -5]], np.float32), *one(1))[0][0]  # a camera behind it: t = 0.75
    assert pr.blocked(np.array([[-1, -0.5, -1]], np.float32), cam, *one(2))[0][0]
    assert not pr.blocked(np.array([[-1, -0.5, -1.5]], np.float32), cam, *one(2))[0][0]
    assert not pr.blocked(np.array([[0, 0, -1]], np.float32), cam, *one(3))[0][0]  # the invalid triangle across the axis
    # a start at the camera (D = 0) and one that is not finite are blocked by nothing
    assert not pr.blocked(np.array([[0, 0, -3], [np.nan, 0, 0]], np.float32), np.repeat(cam, 2, axis=0), pr.HAND_VERTICES, pr.HAND_TRIANGLES)[0].any()


def test_all_hand_cases_against_all_hand_views_in_one_call_is_the_sum_of_single_views():
    points, normals = pr.hand_points()
    color, weight, poses, intr = pr.hand_stack()
    for kw in (dict(), dict(bias=0.5, sides="both", power=2), dict(mode="best", power=1, cos_min=0.5)):
        one = pr.project(points, normals, color, weight, poses, intr, pr.HAND_VERTICES, pr.HAND_TRIANGLES, **kw)
        acc_c, acc_w = np.zeros_like(one[0]), np.zeros_like(one[1])
        for v in range(len(color)):
            pr.integrate(acc_c, acc_w, points, normals, color[v:v + 1], weight[v:v + 1], poses[v:v + 1], intr[v:v + 1], pr.HAND_VERTICES,
                         pr.HAND_TRIANGLES, **kw)
        assert np.array_equal(one[0], acc_c, equal_nan=True) and np.array_equal(one[1], acc_w, equal_nan=True)
        assert one[1].any()


@pytest.mark.parametrize("mode", pr.MODES)
def test_batches_leave_the_bits_of_one_call(sphere, mode):
    s, sv = sphere, sphere["sv"]
    kw = dict(s["kw"], mode=mode)
    args = lambda a, b: (sv["color"][a:b], sv["weight"][a:b], sv["poses"][a:b], sv["intrinsics"][a:b], s["v"], s["t"])  # noqa: E731
    one = pr.project(s["v"], s["n"], *args(0, 14), **kw)
    N = len(s["v"])
    two, each = (np.zeros((N, 3), np.float32), np.zeros(N, np.float32)), (np.zeros((N, 3), np.float32), np.zeros(N, np.float32))
    pr.integrate(*two, s["v"], s["n"], *args(0, 8), **kw)
    pr.integrate(*two, s["v"], s["n"], *args(8, 14), **kw)
    for v in range(14):
        pr.integrate(*each, s["v"], s["n"], *args(v, v + 1), **kw)
    for a, b, c in zip(one[:2], two, each):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    if mode == "blend":
        assert np.array_equal(one[0], s["acc32"][0]) and np.array_equal(one[1], s["acc32"][1])


def test_best_keeps_the_earliest_of_equal_views():
    view = pr.hand_views()["ramp"]
    colors = np.stack([view["color"], view["color"] + np.float32(0.125), view["color"] + np.float32(0.25)])
    poses, intr = np.stack([view["pose"]] * 3), np.stack([view["intrinsics"]] * 3)
    pts, nrm = np.array([pr.AXIS, pr.OFF], np.float32), np.array([pr.TILTED, pr.TOWARDS], np.float32)
    acc_c, acc_w, _ = pr.project(pts, nrm, colors, None, poses, intr, pr.HAND_VERTICES, pr.HAND_TRIANGLES, mode="best", power=2)
    c08 = np.float32(0.8)
    assert acc_w[0] == c08 * c08 and np.array_equal(acc_c[0], pr.hand_color(17))  # view 0, not 1 or 2, and the colour is not weighted
    assert np.array_equal(acc_c[1], pr.hand_color(19.25))
    # a later view wins only with a LARGER weight
    weight = np.stack([np.full((pr.HAND_H, pr.HAND_W), w, np.float32) for w in (1.0, 2.0, 2.0)])
    acc_c, acc_w, _ = pr.project(pts, nrm, colors, weight, poses, intr, pr.HAND_VERTICES, pr.HAND_TRIANGLES, mode="best", power=2)
    assert acc_w[0] == (c08 * c08) * np.float32(2) and np.array_equal(acc_c[0], pr.hand_color(17) + np.float32(0.125))
    col, seen, totals = pr.finalize(acc_c, acc_w, 1e-6, "best", np.zeros_like(acc_c))
    assert np.array_equal(col[0], pr.hand_color(17) + np.float32(0.125)) and totals == (2, 0) and seen.all()


def test_finalize_divides_clamps_and_leaves_the_fallback():
    acc_w = np.array([2.0, 0.5, 0.0, np.nan, 1.0, 1.0], np.float32)
    acc_c = np.array([[1, 0.5, 3], [9, 9, 9], [0, 0, 0], [1, 1, 1], [-1, 0.25, 2], [np.nan, 0.5, 0.5]], np.float32)
    fallback = np.full((6, 3), 0.3, np.float32)
    col, seen, totals = pr.finalize(acc_c, acc_w, 1.0, "blend", fallback)
    assert seen.tolist() == [1, 0, 0, 0, 1, 1] and totals == (3, 3)
    assert np.array_equal(col[0], np.array([0.5, 0.25, 1.0], np.float32)) and np.array_equal(col[4], np.array([0, 0.25, 1.0], np.float32))
    assert np.array_equal(col[[1, 2, 3]], fallback[[1, 2, 3]])
    assert np.array_equal(col[5], np.array([0, 0.5, 0.5], np.float32))  # fmaxf(NaN, 0) is 0
    col, seen, totals = pr.finalize(acc_c, acc_w, 0.5, "best", fallback)
    assert seen.tolist() == [1, 1, 0, 0, 1, 1] and np.array_equal(col[0], np.array([1, 0.5, 1], np.float32)) and np.array_equal(col[1], np.ones(3, np.float32))


# --------------------------------------------------------------------------------------------------- float32 against float64
def rounding_bound(sv, radius=0.95):
    """What float32 rounding can do to the blended colour of a point whose views take the same decisions in both precisions, from the
    operation count (u = 2^-24 per operation).  |d| <= D = distance + radius + 0.04 (the ball is off centre).  A component of q is
    three products and two sums of numbers bounded by sqrt 3 D on top of the rounding of d: |dq| <= 6 u sqrt 3 D.  q_z >= Z = distance -
    radius - 0.04.  x - cx = fx q_x / q_z with |q_x / q_z| <= tan(half the field of view) = (W / 2) / fx: |dx| <= fx |dq| (1 + tan) / Z
    plus three roundings (product, quotient, sum) of numbers below W: e_x = fx |dq| (1 + tan) / Z + 3 u W.  The bilinear mix moves with
    the fractional position by at most the difference of neighbouring pixels, <= 1 for colours in [0, 1], along each image axis: 2 e_x,
    plus 7 u for its own seven operations and 4 u for the weights' (they sum to 1).  The view weight c c wp is 8 operations for c, two
    products and the mix wp (7): relative 17 u.  A quotient of sums of V terms, sum w C / sum w, moves by the error of C plus twice the
    relative error of the weights plus the roundings of both sums (V each) and the quotient: 2 e_x + (11 + 2 * 17 + 2 V + 1) u."""
    V, W = sv["color"].shape[0], sv["color"].shape[2]
    D, Z = sv["distance"] + radius + 0.04, sv["distance"] - radius - 0.04
    dq = 6 * U * np.sqrt(3.0) * D
    e_x = sv["fx"] * dq * (1 + (W / 2) / sv["fx"]) / Z + 3 * U * W
    return 2 * e_x + (11 + 34 + 2 * V + 1) * U


def test_float32_against_the_float64_twin(sphere):
    """The float32 restatement stays within the derived bound of its float64 twin on every point whose views all take the same
    decisions in both (the kept masks of step 9 agree); those are nearly all points."""
    kept32 = np.stack([t["kept"] for t in sphere["t32"]])
    kept64 = np.stack([t["kept"] for t in sphere["t64"]])
    same = (kept32 == kept64).all(axis=0)
    assert same.mean() >= 0.98, same.mean()
    c32, w32, _ = sphere["acc32"]
    c64, w64, _ = sphere["acc64"]
    assert (w64[same] > 0).all()
    err = np.abs(c32.astype(np.float64) / w32.astype(np.float64)[:, None] - c64 / w64[:, None])[same]
    bound = rounding_bound(sphere["sv"])
    print("blended colour: the largest |float32 - float64| %.3e, bound %.3e (%.0f u); %d of %d points compared"
          % (err.max(), bound, bound / U, int(same.sum()), len(same)))
    assert err.max() <= bound
    assert err.max() > 0  # the twin is not the same computation


# --------------------------------------------------------------------------------------------------- end to end
def test_the_patterned_sphere_is_recovered_within_the_derived_bound(sphere):
    """14 images of the sphere mesh, coloured 0.5 + 0.5 sin(k hit), projected back onto its vertices: every vertex is seen and gets the
    pattern back within 0.5 k sqrt 2 (r / fx) / cos_min (mesh_project_restatement.sphere_bound) plus float slack.  Derived bound
    0.19808, measured maximum 0.005867 (profiles/mesh_project_checks.txt)."""
    acc_c, acc_w, ratio = sphere["acc32"]
    col, seen, totals = pr.finalize(acc_c, acc_w, 1e-6, "blend", np.full_like(acc_c, -1.0))
    assert totals == (len(seen), 0) and seen.all()
    err = np.abs(col.astype(np.float64) - pr.pattern(sphere["v"])).max()
    bound = pr.sphere_bound(sphere["sv"]["fx"], sphere["sv"]["distance"])
    print("patterned sphere: derived bound %.5f, measured maximum %.6f, unseen %d, views per vertex %d .. %d"
          % (bound, err, totals[1], int(np.stack([t["kept"] for t in sphere["t32"]]).sum(axis=0).min()),
             int(np.stack([t["kept"] for t in sphere["t32"]]).sum(axis=0).max())))
    assert err <= bound + 1e-5
    # the occlusion test matters: without the mesh the far side's cameras are only held off by the facing test; with sides="both" and
    # no mesh, views through the ball reach the vertices and the pattern is lost
    sv = sphere["sv"]
    through = pr.project(sphere["v"], sphere["n"], sv["color"], sv["weight"], sv["poses"], sv["intrinsics"], sphere["v"], sphere["t"][:0],
                         **dict(sphere["kw"], sides="both"))
    c2, _, _ = pr.finalize(through[0], through[1], 1e-6, "blend", np.zeros_like(acc_c))
    assert np.abs(c2.astype(np.float64) - pr.pattern(sphere["v"])).max() > bound
    both = pr.project(sphere["v"], sphere["n"], sv["color"], sv["weight"], sv["poses"], sv["intrinsics"], sphere["v"], sphere["t"],
                      **dict(sphere["kw"], sides="both"))
    assert np.array_equal(both[1], acc_w) and np.array_equal(both[0], acc_c)  # the mesh blocks exactly the views from behind


def test_the_edge_on_margin_of_the_fixtures_the_gpu_tests_compare_across_grids(sphere):
    """tests/test_hip_mesh_project.py runs the sphere fixture at G = 1, 4 and 16 and over a shifted box and expects the same bytes: every
    (ray, triangle) pair that is not missed is far from edge-on (mesh_expose_restatement.DET_BOUND).  blocked()'s measure is det_ratio's:
    on rays whose direction is exact in float32 the two agree."""
    assert sphere["acc32"][2] > 1e3 * pr.DET_BOUND, sphere["acc32"][2]
    o = np.array([[0.25, 0.5, -3], [1, 0.5, -1]], np.float32)
    cam = np.array([[0.5, 0.25, 1], [0, 0, -3]], np.float32)
    v, t = sphere["v"], sphere["t"]
    _, mine = pr.blocked(o, cam, v, t)
    d = cam - o  # exact
    tm = xr.rr.hit_matrix(o, d, v, t)[0]
    rows, cols = np.nonzero(~np.isnan(tm))
    assert len(rows) and mine == float(xr.det_ratio(o, d, v, t, rows, cols).min())


def test_a_quad_shadows_the_plane_below_it():
    oc = pr.occluder_case()
    acc_c, acc_w, _ = pr.project(oc["points"], oc["normals"], oc["color"], None, oc["poses"], oc["intrinsics"], oc["vertices"],
                                 oc["triangles"], cos_min=0.2, power=2, bias=1e-3)
    sh = oc["shadowed"]
    assert 0 < sh.sum() < len(sh)
    assert (acc_w[sh] == 0).all() and (acc_c[sh] == 0).all() and (acc_w[~sh] > 0).all()
    fallback = np.full((len(sh), 3), 0.875, np.float32)
    col, seen, totals = pr.finalize(acc_c, acc_w, 1e-6, "blend", fallback)
    assert totals == (int((~sh).sum()), int(sh.sum())) and np.array_equal(seen.astype(bool), ~sh)
    assert np.array_equal(col[sh], fallback[sh])
    assert np.abs(col[~sh] - np.array([0.25, 0.5, 0.75], np.float32)).max() <= 4 * U
    # without the quad nothing is shadowed
    _, w2, _ = pr.project(oc["points"], oc["normals"], oc["color"], None, oc["poses"], oc["intrinsics"], oc["vertices"], oc["triangles"][:2],
                          cos_min=0.2, power=2, bias=1e-3)
    assert (w2 > 0).all()
