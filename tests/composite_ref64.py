"""Float64 restatement of the training compositing (k_composite_fwd_wave / k_composite_bwd_wave of csrc/raymarching.hip, with
their epilogue, objective and group variants), a per-element error bound for the float32 kernels, and scripted inputs.
Plain numpy, one sequential loop over the samples of a ray; nothing here imports the library under test.

FORMULAS (from the float32 inputs widened to float64; per ray, samples j = 0 .. L-1, T_0 = 1, t = 0)

    alpha_j = 1 - exp(-sigma_j d0_j)     w_j = alpha_j T_j     T_{j+1} = T_j (1 - alpha_j)     t_j = t_{j-1} + d1_j
    ws = sum w_j        depth = sum w_j t_j        image_k = sum w_j c_jk
    a ray with num == 0 or offset + num >= budget gives zeros (budget = M, or min(M, max(*device_budget, 0)))
    epilogue:  image_k += (1 - ws) bg_k        depth = max(depth - near, 0) / (far - near + eps)

    backward, from the ws / image THE KERNEL IS HANDED (float32, widened), g = d/d image, gws = d/d ws:
    epilogue:  image_k -= (1 - ws) bg_k        gws -= sum_k g_k bg_k
    r_jk = sum_{i<=j} w_i c_ik     s_j = sum_{i<=j} w_i
    grad_sigma_j = d0_j ( sum_k g_k (T_{j+1} c_jk - (image_k - r_jk)) + gws (T_{j+1} - (ws - s_j)) )
    grad_rgb_jk  = g_k w_j

    objective:  S = (sum (I_t - I_s)^2, sum dF^2, sum dsigma^2, sum dc^2)   norm_i = sqrt(S_i)
    coef_i = rate_i / norm_i (0 when norm_i == 0)      loss = sum(extra) + sum_i rate_i norm_i
    g_image = coef_0 up (I_s - I_t)    g_fea = coef_1 up dF (+ coef_2 up dsigma in column 0)    g_col = coef_3 up dc

BOUND (u = 2^-24, the unit roundoff of float32; every line follows the kernel's operation order)

  alpha.  x = fl(sigma d0) carries u x relative; __expf is v_exp_f32 after a float32 multiply by log2 e: the multiply moves the
  exponent by 2 u x relatively, the instruction is good to one ulp (<= 2 u relative).  So |E - e^-x| <= e^-x (3 u x + 2 u)
  <= (3 / e + 2) u because x e^-x <= 1 / e, and 1 - E rounds once more (<= u): |alpha_k - alpha| <= EA = 5 u, ABSOLUTE.
  q = 1 - alpha is formed by another subtraction: |q_k - q| <= EQ = 6 u.  (A relative statement is impossible: the tiny-sigma rays
  have alpha_k = 0 and the opaque samples q_k = 0.)

  T.  A product of factors in [0, 1] with absolute errors EQ moves by at most EQ * Tdot_j, Tdot_j = sum_{i<j} prod_{l<j, l!=i} q_l
  (recursion Tdot_{j+1} = Tdot_j q_j + T_j, evaluated with q + EQ).  The wave forms it with a 6-level Hillis-Steele scan, one
  multiply by the carry and one carry update per earlier chunk: (8 + chunk) roundings.
      eT_j = EQ Tdot_j + (8 + chunk_j) u T_j                                 (same form for the post-update T_{j+1} of the backward)
  w.  ew_j = EA (T_j + eT_j) + alpha_j eT_j + u w_j.
  t.  6 scan levels, the carry add, one carry per chunk: et_j = (8 + chunk_j) u t_j  (d1 >= 0).

  forward sums.  A lane adds one product per chunk (n_chunk of them), the wave reduction adds 6 levels:
      e(sum w x) = sum ew_j |x_j| (+ w_j et_j for x = t) + (n_chunk + 7) u sum (w_j + ew_j) |x_j|
  epilogue.  1 - ws, the product with bg and the add round once each: e_image += e_ws bg + 3 u (|image| + |1 - ws| bg);
  depth: (e_depth + u |depth - near|) / D (1 + 4 u) + 4 u depth_out with D = far - near + eps (two roundings, one for the division).

  backward.  The un-blend rounds three times in float32 on the float32 ws / image inputs: eF_k = 3 u (|image_k| + |1 - ws| bg_k);
  gws: e_gws = 4 u (|gws| + sum |g_k| bg_k).  Prefix sums: product, 6 scan levels, carry add, one carry per chunk:
      er_jk = sum_{i<=j} ew_i c_ik + (9 + chunk_j) u sum_{i<=j} (w_i + ew_i) c_ik
  Each of the four terms g (T c - (F - r)) rounds in T c, F - r, the outer difference, the product with g; three adds and the
  product with d0 follow: 8 u on the magnitude A_k = T c_k + |F_k - r_jk|.  With prop_k = eT c_k + eF_k + er_jk:
      e(grad_sigma_j) = d0_j sum_{k in rgb, ws} ( |g_k| (prop_k + 8 u (A_k + prop_k)) + eg_k (A_k + prop_k) )
      e(grad_rgb_jk)  = |g_k| (ew_j + u w_j) + eg_k (w_j + ew_j)
  eg_k is the error of the incoming gradient: 0 when it is an input; with the objective riding, g_k = coef up (I_s - I_t) rounds
  three times and inherits the coefficient's relative error: eg_k = |g_k| (3 u + rel(coef)).

  objective sums.  n non-negative terms summed in ANY order are off by at most (n - 1) u relatively; the difference and the square
  add 3 u, the block / partial reductions are part of "any order": e_S = (n + 24) u S.  The image term also inherits the forward's
  error: + sum (2 |d| e_image + e_image^2).  norm = sqrt(S): e_S / (2 S) + u relative; coef = rate / norm: one more rounding;
  rel(coef) = e_S / (2 S) (1 + e_S / S) + 3 u.  loss: sum rate_i e_norm_i + (n_extra + 8) u (sum |extra| + sum rate_i norm_i).
  g_fea / g_col: |g| (rel(coef) + 4 u), column 0 of g_fea the sum of two such terms.

  Every bound that is not required to be exact also gets TINY = 2^-120 (denormal intermediates may be flushed).  Second-order
  terms are carried where they can matter (magnitudes are taken as value + error).  tests/test_composite_ref64.py checks that two
  float32 restatements (the wave order and the sequential order) stay inside and that ten modelled single faults do not."""
import copy
import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
EA = 5 * U
EQ = 6 * U
TINY = 2.0 ** -120
WAVE = 64
RAYS_PER_GROUP = 4  # kBlock / kWave of csrc/raymarching.hip: one wave per ray, 256 threads per workgroup
PAD = 160           # sentinel slots behind M samples / N rays in the buffers the tests hand to the kernels

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193)
LONG = 1024
REGIMES = ("random", "zero", "tiny", "opaque", "last", "thin")
OPAQUE_AT = {1: 0, 2: 1, 63: 31, 64: 63, 65: 64, 127: 63, 128: 64, 129: 100, 192: 63, 193: 64}

Out = namedtuple("Out", "y bound")


# ---------------------------------------------------------------------------------------------- one ray
def trace(sig, rgb, dl, records=True):
    """The sequential loop.  sig [..., L], rgb [..., L, 3] (leading axes: independent copies of the ray, for finite differences),
    dl [L, 2]; float64.  Returns the sums, their error forms and (records) the per-sample quantities the backward needs."""
    L = dl.shape[0]
    lead = sig.shape[:-1]
    n_chunk = (L + WAVE - 1) // WAVE
    T, Tdot, t = np.ones(lead), np.zeros(lead), 0.0
    z, z3 = np.zeros(lead), np.zeros(lead + (3,))
    ws, dep, img = z.copy(), z.copy(), z3.copy()
    e_ws, e_dep, e_img = z.copy(), z.copy(), z3.copy()
    m_ws, m_dep, m_img = z.copy(), z.copy(), z3.copy()
    rec = {k: np.zeros(lead + (L,) + s) for k, s in (("w", ()), ("ew", ()), ("Tpost", ()), ("eTpost", ()), ("s", ()), ("es", ()),
                                                     ("r", (3,)), ("er", (3,)))} if records else None
    pe_s, pm_s, pe_r, pm_r = z.copy(), z.copy(), z3.copy(), z3.copy()
    for j in range(L):
        ch = j // WAVE
        x = sig[..., j] * dl[j, 0]
        a = -np.expm1(-x)
        q = np.exp(-x)
        qb = np.minimum(1.0, q + EQ)
        eT = EQ * Tdot + (8 + ch) * U * T
        Tb = T + eT
        w = a * T
        ew = EA * Tb + a * eT + U * a * Tb
        wb = w + ew
        t = t + dl[j, 1]
        et = (8 + ch) * U * t
        c = rgb[..., j, :]
        ws, e_ws, m_ws = ws + w, e_ws + ew, m_ws + wb
        dep, e_dep, m_dep = dep + w * t, e_dep + ew * t + wb * et, m_dep + wb * (t + et)
        img, e_img, m_img = img + w[..., None] * c, e_img + ew[..., None] * np.abs(c), m_img + wb[..., None] * np.abs(c)
        Tdot = Tdot * qb + Tb
        T = T * q
        if records:
            pe_s, pm_s = pe_s + ew, pm_s + wb
            pe_r, pm_r = pe_r + ew[..., None] * np.abs(c), pm_r + wb[..., None] * np.abs(c)
            rec["w"][..., j], rec["ew"][..., j] = w, ew
            rec["Tpost"][..., j], rec["eTpost"][..., j] = T, EQ * Tdot + (8 + ch) * U * T
            rec["s"][..., j], rec["es"][..., j] = ws, pe_s + (9 + ch) * U * pm_s
            rec["r"][..., j, :], rec["er"][..., j, :] = img, pe_r + (9 + ch) * U * pm_r
    k = (n_chunk + 7) * U
    return dict(ws=ws, depth=dep, image=img, e_ws=e_ws + k * m_ws, e_depth=e_dep + k * m_dep, e_image=e_img + k * m_img, rec=rec)


def _bg_rows(bg, N):
    """bg as [N, 3] float64 by ray index (scalar: broadcast); None: no epilogue"""
    if bg is None:
        return None
    if np.isscalar(bg):
        return np.full((N, 3), float(np.float32(bg)))
    return np.asarray(bg, np.float64).reshape(N, 3)


def logical_budget(M, budget):
    return M if budget is None else min(M, max(int(budget), 0))


def kept(case, budget=None):
    """[N] bool by ROW: the ray is composited (not empty, not dropped)"""
    lim = logical_budget(case.M, budget)
    off, num = case.rays[:, 1].astype(np.int64), case.rays[:, 2].astype(np.int64)
    return (num != 0) & (off + num < lim)


# ---------------------------------------------------------------------------------------------- forward
def forward(case, budget=None, bg=None, depth_eps=None, sigmas=None, rgbs=None):
    """-> dict ws [N], depth [N], image [N, 3] of Out(value, bound), by ray INDEX.  bg None: the plain form (budget must be None);
    else the epilogue form with case.nears / case.fars and float32 depth_eps."""
    N = case.N
    sig = (case.sigmas if sigmas is None else sigmas).astype(np.float64)
    rgb = (case.rgbs if rgbs is None else rgbs).astype(np.float64)
    dl = case.deltas.astype(np.float64)
    bgr = _bg_rows(bg, N)
    keep = kept(case, budget)
    ws, dep, img = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    b_ws, b_dep, b_img = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    for n in range(N):
        idx, off, num = (int(v) for v in case.rays[n])
        if keep[n]:
            tr = trace(sig[off:off + num], rgb[off:off + num], dl[off:off + num], records=False)
            ws[idx], dep[idx], img[idx] = tr["ws"], tr["depth"], tr["image"]
            b_ws[idx], b_dep[idx], b_img[idx] = tr["e_ws"] + TINY, tr["e_depth"] + TINY, tr["e_image"] + TINY
        if bgr is not None:
            tt = 1.0 - ws[idx]
            b_img[idx] = b_img[idx] + b_ws[idx] * bgr[idx] + (3 * U * (np.abs(img[idx]) + abs(tt) * bgr[idx]) if keep[n] else 0.0)
            img[idx] = img[idx] + tt * bgr[idx]
            near, far = float(case.nears[idx]), float(case.fars[idx])
            D = (far - near) + float(np.float32(depth_eps))
            d0 = dep[idx] - near
            out = max(d0, 0.0) / D
            b_dep[idx] = ((b_dep[idx] + U * abs(d0)) / D * (1 + 4 * U) + 4 * U * out) if (keep[n] or out != 0.0) else 0.0
            dep[idx] = out
    return dict(ws=Out(ws, b_ws), depth=Out(dep, b_dep), image=Out(img, b_img))


# ---------------------------------------------------------------------------------------------- backward
def backward(case, ws_in, image_in, gws, gimg, budget=None, bg=None, e_g=None):
    """ws_in [N], image_in [N, 3]: the float32 buffers the kernel is handed (by ray index); gws [N] or None; gimg [N, 3]; e_g [N, 3]:
    error of gimg (objective form).  -> grad_sigmas Out [Mphys], grad_rgbs Out [Mphys, 3], owned [Mphys] bool (slots of kept rays;
    everything else is 0 with bound 0: `fresh` writes exactly that, the other forms leave those slots alone)."""
    N, Mp = case.N, case.sigmas.shape[0]
    sig, rgb, dl = case.sigmas.astype(np.float64), case.rgbs.astype(np.float64), case.deltas.astype(np.float64)
    bgr = _bg_rows(bg, N)
    keep = kept(case, budget)
    wsF_all, F_all = np.asarray(ws_in, np.float64), np.asarray(image_in, np.float64).reshape(N, 3)
    gimg = np.asarray(gimg, np.float64).reshape(N, 3)
    gs, b_gs, owned = np.zeros(Mp), np.zeros(Mp), np.zeros(Mp, bool)
    gr, b_gr = np.zeros((Mp, 3)), np.zeros((Mp, 3))
    for n in range(N):
        idx, off, num = (int(v) for v in case.rays[n])
        if not keep[n]:
            continue
        sl = slice(off, off + num)
        rec = trace(sig[sl], rgb[sl], dl[sl])["rec"]
        g = gimg[idx]
        eg = np.zeros(3) if e_g is None else np.asarray(e_g, np.float64).reshape(N, 3)[idx]
        gw = 0.0 if gws is None else float(gws[idx])
        F, wsF, eF, egw = F_all[idx].copy(), wsF_all[idx], np.zeros(3), 0.0
        if bgr is not None:
            tt = 1.0 - wsF
            eF = 3 * U * (np.abs(F) + abs(tt) * bgr[idx])
            egw = 4 * U * (abs(gw) + np.sum(np.abs(g) * bgr[idx])) + np.sum(eg * bgr[idx])
            F = F - tt * bgr[idx]
            gw = gw - np.sum(g * bgr[idx])
        c, d0 = rgb[sl], dl[sl, 0]
        Tp, eTp = rec["Tpost"], rec["eTpost"]
        term = Tp[:, None] * c - (F[None, :] - rec["r"])
        term_w = Tp - (wsF - rec["s"])
        gs[sl] = d0 * (term @ g + gw * term_w)
        A = (Tp + eTp)[:, None] * c + np.abs(F[None, :] - rec["r"])
        prop = eTp[:, None] * c + eF[None, :] + rec["er"]
        A_w = (Tp + eTp) + np.abs(wsF - rec["s"])
        prop_w = eTp + rec["es"]
        b_gs[sl] = d0 * ((prop + 8 * U * (A + prop)) @ np.abs(g) + (A + prop) @ eg
                         + abs(gw) * (prop_w + 8 * U * (A_w + prop_w)) + egw * (A_w + prop_w)) + TINY
        gr[sl] = rec["w"][:, None] * g[None, :]
        b_gr[sl] = (rec["ew"] + U * rec["w"])[:, None] * np.abs(g)[None, :] + (rec["w"] + rec["ew"])[:, None] * eg[None, :] + TINY
        owned[sl] = True
    return Out(gs, b_gs), Out(gr, b_gr), owned


# ---------------------------------------------------------------------------------------------- objective
def objective_inputs(case, rows, zero_term=None, seed=5):
    """teacher image [N, 3], feature rows [rows, 16] x2, colour rows [rows, 3] x2, rates [4], extra [7], upstream [1] (float32);
    zero_term: 'col' makes the student's colours the teacher's (that norm is exactly 0)"""
    rng = np.random.default_rng(seed + rows)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    o = dict(img_t=f32(rng.uniform(0, 1, (case.N, 3))), fea_s=f32(rng.normal(0, 1, (rows, 16))), fea_t=f32(rng.normal(0, 1, (rows, 16))),
             col_s=f32(rng.uniform(0, 1, (rows, 3))), col_t=f32(rng.uniform(0, 1, (rows, 3))),
             rates=f32([1.0, 0.0625, 0.25, 0.5]), extra=f32(rng.uniform(0, 1e-3, 7)), upstream=f32([0.75]))
    if zero_term == "col":
        o["col_s"] = o["col_t"].copy()
    return o


def objective_sums(image, e_image, ob):
    """image Out-like (float64 forward, blended) -> S Out [4]"""
    d_img = ob["img_t"].astype(np.float64) - image
    d_fea = ob["fea_s"].astype(np.float64) - ob["fea_t"].astype(np.float64)
    d_col = ob["col_s"].astype(np.float64) - ob["col_t"].astype(np.float64)
    S = np.array([np.sum(d_img ** 2), np.sum(d_fea ** 2), np.sum(d_fea[:, 0] ** 2), np.sum(d_col ** 2)])
    n = np.array([d_img.size, d_fea.size, d_fea.shape[0], d_col.size])
    b = (n + 24) * U * S
    b[0] += np.sum(2 * np.abs(d_img) * e_image + e_image ** 2) * (1 + (n[0] + 24) * U)
    return Out(S, b + TINY * (S > 0))


def objective_finish(S, ob, with_extra=True):
    """S Out [4] -> norms, coef, loss (Out each) and rel(coef) [4]"""
    rates = ob["rates"].astype(np.float64)
    nrm = np.sqrt(S.y)
    pos = S.y > 0
    relS = np.where(pos, S.bound / np.where(pos, S.y, 1.0), 0.0)
    e_nrm = nrm * (relS / 2 * (1 + relS) + U)
    coef = np.where(pos, rates / np.where(pos, nrm, 1.0), 0.0)
    relc = np.where(pos, relS / 2 * (1 + relS) + 3 * U, 0.0)
    extra = ob["extra"].astype(np.float64) if with_extra else np.zeros(0)
    loss = extra.sum() + np.sum(rates * nrm)
    e_loss = np.sum(rates * e_nrm) + (extra.size + 8) * U * (np.abs(extra).sum() + np.sum(rates * nrm)) + TINY
    return Out(nrm, e_nrm), Out(coef, np.abs(coef) * relc), Out(np.array([loss]), np.array([e_loss])), relc


def objective_grads(coef, relc, ob, image_in):
    """coef [4] float64 (what the backward used or should have formed), relc [4] its relative error, image_in [N, 3] the float32
    image the backward is handed -> g_image, e_g_image [N, 3]; g_fea Out [rows, 16]; g_col Out [rows, 3]"""
    up = float(ob["upstream"][0])
    d_img = np.asarray(image_in, np.float64).reshape(-1, 3) - ob["img_t"].astype(np.float64)
    g_img = coef[0] * up * d_img
    e_img = np.abs(g_img) * (3 * U + relc[0])
    d_fea = ob["fea_s"].astype(np.float64) - ob["fea_t"].astype(np.float64)
    g_fea = coef[1] * up * d_fea
    b_fea = np.abs(g_fea) * (relc[1] + 4 * U)
    g_fea[:, 0] += coef[2] * up * d_fea[:, 0]
    b_fea[:, 0] += np.abs(coef[2] * up * d_fea[:, 0]) * (relc[2] + 4 * U) + U * np.abs(g_fea[:, 0])
    d_col = ob["col_s"].astype(np.float64) - ob["col_t"].astype(np.float64)
    g_col = coef[3] * up * d_col
    return g_img, e_img, Out(g_fea, b_fea + TINY), Out(g_col, np.abs(g_col) * (relc[3] + 4 * U) + TINY * (coef[3] != 0))


# ---------------------------------------------------------------------------------------------- scripted inputs
class Case:
    pass


def _ray_samples(regime, L, rid):
    """(sigma [L], rgb [L, 3], deltas [L, 2]) float32 of one scripted ray"""
    rng = np.random.default_rng(1000 + rid)
    d = 1.7 / 1024 * (1 + rid % 4)
    dl = (d * rng.uniform(0.5, 1.5, (L, 2))).astype(np.float32)
    rgb = rng.uniform(0, 1, (L, 3))
    pick = rng.uniform(0, 1, (L, 3))
    rgb[pick < 0.1], rgb[pick > 0.9] = 0.0, 1.0
    thin = np.exp(rng.uniform(-2, 2, L))
    if regime == "random":
        sig = np.exp(rng.uniform(-2, 7, L))
    elif regime == "zero":
        sig = np.zeros(L)
    elif regime == "tiny":
        sig = rng.uniform(0.1, 1, L) * 2.0 ** -26 / np.maximum(dl[:, 0].astype(np.float64), 1e-30)
    elif regime == "opaque":
        sig = thin
        if L:
            sig[OPAQUE_AT[L]] = 2.0e5  # sigma d0 >= 166: exp underflows float32, 1 - alpha is exactly 0
    elif regime == "last":
        sig = thin * 1e-2
        if L:
            sig[-1] = 10.0 / float(dl[-1, 0])
    elif regime == "thin":
        sig = thin
    else:
        raise ValueError(regime)
    return sig.astype(np.float32), rgb.astype(np.float32), dl


def _rows():
    """(regime, length) by row: every regime on every length, the long ray, three budget-edge rays before a last empty one;
    empty rays first, in the middle and last"""
    grid = [(r, L) for r in REGIMES for L in LENGTHS]
    order = np.random.default_rng(3).permutation(len(grid))
    rows = [grid[i] for i in order] + [("thin", LONG)]
    empties = [i for i, (_, L) in enumerate(rows) if L == 0]
    first, mid, last = (rows[i] for i in empties[:3])
    rows = [r for i, r in enumerate(rows) if i not in empties[:3]]
    rows = [first] + rows[:len(rows) // 2] + [mid] + rows[len(rows) // 2:]
    return rows + [("random", 63), ("thin", 1), ("thin", 2), last]


def _build(label, rows, kind):
    """kind 'fresh': index = row, offsets = exclusive prefix sum in row order.  'perm': index a non-identity permutation, the rays'
    samples laid out in another shuffled order.  In both the three rays before the last row end at M - 1, M and M + 2."""
    N = len(rows)
    rng = np.random.default_rng(11)
    rays_data = [_ray_samples(reg, L, rid) for rid, (reg, L) in enumerate(rows)]
    if kind == "fresh" or N < 8:
        layout = list(range(N))
    else:
        layout = list(rng.permutation(N - 4)) + [N - 4, N - 3, N - 2, N - 1]
    index = np.arange(N) if kind == "fresh" else np.roll(rng.permutation(N), 1)
    if kind != "fresh" and np.array_equal(index, np.arange(N)):
        index = index[::-1].copy()
    offs, pos = np.zeros(N, np.int64), 0
    for r in layout:
        offs[r] = pos
        pos += rows[r][1]
    total = pos
    c = Case()
    c.label, c.kind, c.N, c.rows = label, kind, N, rows
    c.total = total
    c.M = int(offs[N - 4] + rows[N - 4][1] + 1) if N >= 8 else total + 1  # the fourth ray from the end stops at M - 1
    Mp = max(c.M, total) + PAD
    c.sigmas, c.rgbs, c.deltas = np.zeros(Mp, np.float32), np.zeros((Mp, 3), np.float32), np.zeros((Mp, 2), np.float32)
    filler = np.random.default_rng(12)
    c.sigmas[:] = filler.uniform(1, 50, Mp)  # slots no ray owns hold plausible values: a kernel that reads them shows
    c.rgbs[:] = filler.uniform(0, 1, (Mp, 3))
    c.deltas[:] = filler.uniform(1e-3, 2e-3, (Mp, 2))
    for r in range(N):
        s, col, dl = rays_data[r]
        c.sigmas[offs[r]:offs[r] + rows[r][1]], c.rgbs[offs[r]:offs[r] + rows[r][1]], c.deltas[offs[r]:offs[r] + rows[r][1]] = s, col, dl
    c.rays = np.stack([index, offs, np.array([L for _, L in rows])], 1).astype(np.int32)
    aux = np.random.default_rng(13)
    c.nears = aux.uniform(0.05, 0.3, N).astype(np.float32)
    c.fars = (c.nears + aux.uniform(1, 3, N)).astype(np.float32)
    c.bg = aux.uniform(0, 1, (N, 3))
    pick = aux.uniform(0, 1, (N, 3))
    c.bg[pick < 0.1], c.bg[pick > 0.9] = 0.0, 1.0
    c.bg = c.bg.astype(np.float32)
    c.gws, c.gimg = aux.normal(0, 1, N).astype(np.float32), aux.normal(0, 1, (N, 3)).astype(np.float32)
    c.depth_eps = 1e-4
    # by INDEX: row, length and regime of the ray that owns an output slot; by SAMPLE: the row that owns it (-1: nobody)
    c.row_of_index = np.argsort(index)
    c.owner = np.full(Mp, -1, np.int64)
    for r in range(N):
        if offs[r] + rows[r][1] <= Mp:
            c.owner[offs[r]:offs[r] + rows[r][1]] = r
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """'perm': the full table, permuted index column, shuffled sample layout (every path but `fresh`); 'fresh': the same rays in row
    order with prefix-sum offsets; 'small': N below the rays-per-workgroup count"""
    if name in ("perm", "fresh"):
        return _build(name, _rows(), name)
    if name == "small":
        return _build(name, [("thin", 65), ("random", 0), ("opaque", 2)], "perm")
    raise KeyError(name)


def with_M(c, M):
    """the same table and samples under another sample budget M (<= the physical size minus PAD)"""
    assert M <= c.sigmas.shape[0]
    c2 = copy.copy(c)
    c2.M = int(M)
    return c2


def empty_like(c):
    """the same index column, every ray empty"""
    c2 = copy.copy(c)
    c2.rays = c.rays.copy()
    c2.rays[:, 1:] = 0
    c2.rows = [(reg, 0) for reg, _ in c.rows]
    c2.owner = np.full_like(c.owner, -1)
    c2.label = "empty"
    return c2


CASE_NAMES = ("perm", "fresh", "small")


def cases():
    return [case(n) for n in CASE_NAMES]


def device_budgets(c):
    """name -> value of the device-side budget word for a full table (None: absent)"""
    mid = int(c.rays[c.N // 2, 1]) if c.kind == "fresh" else c.M // 2
    return {"absent": None, "below": mid, "above": c.M + 100, "zero": 0, "negative": -7}


def assert_coverage(c):
    """everything the scripted inputs promise, read back from the table and the sample buffers themselves"""
    rays, N = c.rays.astype(np.int64), c.N
    idx, off, num = rays[:, 0], rays[:, 1], rays[:, 2]
    assert sorted(idx) == list(range(N))
    if c.kind == "fresh":
        assert np.array_equal(idx, np.arange(N)) and np.array_equal(off, np.concatenate([[0], np.cumsum(num)[:-1]]))
    else:
        assert not np.array_equal(idx, np.arange(N)), "index column must be a non-identity permutation"
    if c.label == "small":
        assert N < RAYS_PER_GROUP and (num == 0).any() and (num > WAVE).any()
        return
    assert N % RAYS_PER_GROUP != 0 and N > RAYS_PER_GROUP
    for L in LENGTHS:
        assert (num == L).sum() >= 2, L
    assert (num == LONG).sum() == 1
    assert num[0] == 0 and num[-1] == 0 and (num[N // 4:3 * N // 4] == 0).any(), "empty rays first, in the middle, last"
    end = off + num
    assert (end == c.M - 1).any() and (end == c.M).any() and (end > c.M).any(), "budget edges M - 1, M, > M"
    assert int(kept(c).sum()) == int((num > 0).sum()) - 2  # exactly the two edge rays are dropped without a device budget
    b = device_budgets(c)
    n_all = int(kept(c).sum())
    assert 0 < int(kept(c, b["below"]).sum()) < n_all and int(kept(c, b["above"]).sum()) == n_all
    assert int(kept(c, b["zero"]).sum()) == 0 and int(kept(c, b["negative"]).sum()) == 0 and b["absent"] is None
    sig, dl, rgb = c.sigmas.astype(np.float64), c.deltas.astype(np.float64), c.rgbs
    seen = {r: set() for r in REGIMES}
    for n in range(N):
        reg, L = c.rows[n]
        assert L == num[n]
        seen[reg].add(L)
        sl = slice(off[n], off[n] + L)
        x = (c.sigmas[sl] * c.deltas[sl, 0]).astype(np.float32)  # the float32 product the kernel forms
        if reg == "zero":
            assert (sig[sl] == 0).all()
        if reg == "tiny" and L:
            assert (x < 2.0 ** -24).all() and (x > 0).all() and (np.float32(1) - np.exp(-x) == 0).all()
        if reg == "opaque" and L:
            p = OPAQUE_AT[L]
            assert np.float32(1) - (np.float32(1) - np.exp(-x[p], dtype=np.float32)) == 0 and (x[:p] < 0.1).all()
        if reg == "last" and L > 1:
            w = trace(sig[sl], rgb[sl].astype(np.float64), dl[sl], records=False)
            a_last = -np.expm1(-sig[sl][-1] * dl[sl][-1, 0])
            assert a_last > 0.999 and w["ws"] > 0.9 and x[:-1].sum() < 0.05, "weight sits in the last sample"
    for reg in REGIMES:
        assert seen[reg] >= set(LENGTHS), reg
    # an opaque sample in the first chunk, in the second chunk, exactly at lanes 63 and 64 of a long ray
    assert OPAQUE_AT[192] == 63 and OPAQUE_AT[193] == 64 and OPAQUE_AT[63] < 63 and 64 < OPAQUE_AT[129] < 128
    own = c.owner >= 0
    assert (c.rgbs[own] == 0).any() and (c.rgbs[own] == 1).any(), "colours include exact 0 and 1"
    assert (c.deltas[own, 0] != c.deltas[own, 1]).all(), "d0 != d1"
    assert (c.bg >= 0).all() and (c.bg <= 1).all() and (c.bg == 0).any() and (c.bg == 1).any()
    f = forward(c, bg=1.0, depth_eps=c.depth_eps)
    assert (f["depth"].y == 0).any() and (f["depth"].y > 0).any(), "depth - near negative for some rays, positive for others"


# ---------------------------------------------------------------------------------------------- reporting
def _where(c, name, flat, shape):
    pos = np.unravel_index(flat, shape)
    i = int(pos[0])
    if name in ("grad_sigmas", "grad_rgbs"):
        r = int(c.owner[i]) if i < c.owner.shape[0] else -1
        if r < 0:
            return "slot %d (unowned)" % i
        return "ray %d sample %d of %d (%s)" % (r, i - int(c.rays[r, 1]), c.rows[r][1], c.rows[r][0])
    if name in ("ws", "depth", "image"):
        r = int(c.row_of_index[i])
        return "ray %d index %d length %d (%s)" % (r, i, c.rows[r][1], c.rows[r][0])
    return "element %s" % (tuple(int(p) for p in pos),)


def ratio(got, out):
    """max over elements of err / bound (0 / 0 = 0, x / 0 = inf), and its flat position"""
    err = np.abs(np.asarray(got, np.float64) - out.y)
    bad = ~np.isfinite(err)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / out.bound)
    q = np.where(bad, np.inf, q)
    if q.size == 0:
        return 0.0, 0
    k = int(np.argmax(q))
    return float(q.reshape(-1)[k]), k


def report(label, c, named):
    """named: [(name, got, Out)] -> ('label | name=ratio @ where ...', worst ratio)"""
    parts, worst = [], 0.0
    for name, got, out in named:
        q, k = ratio(got, out)
        worst = max(worst, q)
        parts.append("%s=%.3f @ %s" % (name, q, _where(c, name, k, out.y.shape) if out.y.size else "-"))
    return "%s | %s" % (label, "; ".join(parts)), worst
