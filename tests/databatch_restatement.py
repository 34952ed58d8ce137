"""numpy restatement of include/pvd_hip_data.h (pvd_image_batch, pvd_error_map_update), independent of the kernels: a vectorised
PCG32, the exponential-race keys in float64, the selection, the cell-to-pixel map in float32, the alpha blend and the EMA.
tests/test_databatch_restatement.py ties each piece to the project's CPU code (oracle.pcg32_stream, pvd.scene, pvd.provider);
tests/test_hip_databatch.py compares the kernels against it."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
_MULT = np.uint64(0x5851F42D4C957F2D)
_M64 = (1 << 64) - 1


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


class Pcg32:
    """PCG32 (XSH-RR 64/32) over arrays: one generator per element of `initstate` (broadcast against `initseq`)."""

    def __init__(self, initstate, initseq=1):
        with np.errstate(over="ignore"):
            initstate, initseq = np.broadcast_arrays(_u64(initstate), _u64(initseq))
            self.inc = (initseq << np.uint64(1)) | np.uint64(1)
            self.state = np.zeros_like(self.inc)
            self.next()
            self.state = self.state + initstate
            self.next()

    def next(self):
        with np.errstate(over="ignore"):
            old = self.state
            self.state = old * _MULT + self.inc
            xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
            rot = (old >> np.uint64(59)).astype(np.uint32)
            return (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))

    def next_float(self):
        return (((self.next() >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)).astype(np.float32)

    def advance(self, delta):
        with np.errstate(over="ignore"):
            delta = np.broadcast_to(_u64(delta), np.broadcast(self.state, _u64(delta)).shape).copy()
            self.state = np.broadcast_to(self.state, delta.shape).copy()
            self.inc = np.broadcast_to(self.inc, delta.shape).copy()
            cur_mult, cur_plus = np.full(delta.shape, _MULT, np.uint64), self.inc.copy()
            acc_mult, acc_plus = np.ones(delta.shape, np.uint64), np.zeros(delta.shape, np.uint64)
            while delta.any():
                odd = (delta & np.uint64(1)).astype(bool)
                acc_mult = np.where(odd, acc_mult * cur_mult, acc_mult)
                acc_plus = np.where(odd, acc_plus * cur_mult + cur_plus, acc_plus)
                cur_plus = (cur_mult + np.uint64(1)) * cur_plus
                cur_mult = cur_mult * cur_mult
                delta = delta >> np.uint64(1)
            self.state = acc_mult * self.state + acc_plus
        return self


def batch_initstate(seed, counter):
    """seed + 0x9E3779B97F4A7C15 * (counter + 1) mod 2^64 (counter: int or array of ints)."""
    if np.ndim(counter) == 0:
        return np.uint64((int(seed) + GOLDEN * (int(counter) + 1)) & _M64)
    return np.array([(int(seed) + GOLDEN * (int(c) + 1)) & _M64 for c in np.asarray(counter).ravel()], np.uint64).reshape(np.shape(counter))


def ray_draws(seed, counter, N):
    """The six draws of each of the N rays: (draw0 uint32 [N], u1, u2 float32 [N], bg float32 [N,3])."""
    g = Pcg32(np.full(N, batch_initstate(seed, counter), np.uint64), 1).advance(8 * np.arange(N, dtype=np.uint64))
    d0 = g.next()
    u1, u2 = g.next_float(), g.next_float()
    bg = np.stack([g.next_float(), g.next_float(), g.next_float()], -1)
    return d0, u1, u2, bg


def cell_uniforms(seed, counter, G):
    """The one draw of each of the G cells (float32; counter may be an array: [.., G])."""
    init = batch_initstate(seed, counter)
    g = Pcg32(np.asarray(init)[..., None], 2).advance(np.arange(G, dtype=np.uint64))
    return g.next_float()


def keys64(weights, u):
    """key_c = w_c / e_c, e_c = 0 - log(1 - u_c), in float64 from the float32 weights and uniforms; 0 where w_c is not > 0."""
    w, u = np.asarray(weights, np.float32).astype(np.float64), np.asarray(u, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = 0.0 - np.log(1.0 - u)
        return np.where(w > 0, w / e, 0.0)


def select(keys, N):
    """The N largest keys' cells, equal keys to the lower cell, ascending ([.., G] -> [.., N])."""
    keys = np.asarray(keys)
    order = np.argsort(-keys, axis=-1, kind="stable")  # stable: among equal keys the lower cell first
    return np.sort(order[..., :N], axis=-1).astype(np.int64)


def cell_to_pixel(cells, u1, u2, H, W, g):
    """get_rays' error_map branch (utils.py:357-381) in float32, every operation rounded."""
    cells = np.asarray(cells, np.int64)
    sx, sy = np.float32(H / g), np.float32(W / g)
    fr = (cells // g).astype(np.float32) * sx + np.asarray(u1, np.float32) * sx
    fc = (cells % g).astype(np.float32) * sy + np.asarray(u2, np.float32) * sy
    row, col = np.minimum(fr.astype(np.int64), H - 1), np.minimum(fc.astype(np.int64), W - 1)
    return row * W + col


def uniform_pixels(d0, H, W):
    return ((d0.astype(np.uint64) * np.uint64(H * W)) >> np.uint64(32)).astype(np.int64)


def blend(pixels_u8, bg):
    """training_target (utils.py:987-995) on bytes: rgb a + bg (1 - a) for RGBA, rgb for RGB, in float32."""
    px = np.asarray(pixels_u8, np.uint8).astype(np.float32) / np.float32(255.0)
    if px.shape[-1] == 3:
        return px
    rgb, a = px[..., :3], px[..., 3:]
    return (rgb * a + np.asarray(bg, np.float32) * (np.float32(1.0) - a)).astype(np.float32)


def ema(old, pred, gt):
    """0.1 old + 0.9 ((d0^2 + d1^2) + d2^2) / 3 in float32."""
    d = np.asarray(pred, np.float32) - np.asarray(gt, np.float32)
    err = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / np.float32(3.0)
    return (np.float32(0.1) * np.asarray(old, np.float32) + np.float32(0.9) * err).astype(np.float32)


def image_batch(images_u8, order, position, counter, seed, N, g=0, cells=None):
    """One batch as pvd_image_batch makes it from state = {position, counter}: dict(view, inds, bg, gt).  `cells` [N] (error-map
    mode: the cells the draw chose, ascending) or None for uniform pixels."""
    V, H, W, C = images_u8.shape
    view = int(order[position % V]) if order is not None else position % V
    d0, u1, u2, bg = ray_draws(seed, counter, N)
    inds = uniform_pixels(d0, H, W) if cells is None else cell_to_pixel(cells, u1, u2, H, W, g)
    px = images_u8[view].reshape(H * W, C)[inds]
    return {"view": view, "inds": inds, "bg": bg, "gt": blend(px, bg)}
