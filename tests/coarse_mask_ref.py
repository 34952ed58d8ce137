"""numpy restatement of the coarse occupancy mask (pvd_occ_coarse_mask) and of the 64-point test the training marcher makes with it
(coarse_confine, csrc/raymarching.hip), plus the grids and rays the two tests of it share (tests/test_march_coarse_mask.py on the CPU
against the oracle's serial walk, tests/test_hip_march_coarse_mask.py on the device).  Not a test module."""
import numpy as np

B = 8  # PVD_COARSE_BLOCK
F32 = np.float32
SQRT3 = 1.7320508075688772


# ------------------------------------------------------------------ Morton order, bitfields
def _spread3(v):
    v = v.astype(np.uint64)
    v = (v * 0x00010001) & 0xFF0000FF
    v = (v * 0x00000101) & 0x0F00F00F
    v = (v * 0x00000011) & 0xC30C30C3
    v = (v * 0x00000005) & 0x49249249
    return v


def morton_of_cells(H):
    """[H,H,H] Morton index of cell (x, y, z)."""
    a = _spread3(np.arange(H))
    return (a[:, None, None] | (a[None, :, None] << 1) | (a[None, None, :] << 2)).astype(np.int64)


def bitfield_of(dense):
    """dense bool [C,H,H,H] (x, y, z) -> Morton-ordered bitfield uint8 [C*H^3/8], bit i of byte n = cell 8n + i (packbits)."""
    C, H = dense.shape[0], dense.shape[1]
    m = morton_of_cells(H).reshape(-1)
    bits = np.zeros((C, H ** 3), np.uint8)
    bits[:, m] = dense.reshape(C, -1)
    return np.packbits(bits.reshape(-1), bitorder="little")


def dense_of(bitfield, C, H):
    bits = np.unpackbits(np.asarray(bitfield, np.uint8), bitorder="little").reshape(C, H ** 3)
    return bits[:, morton_of_cells(H).reshape(-1)].reshape(C, H, H, H).astype(bool)


def coarse_mask(bitfield, C, H):
    """uint8 [C*(H/8)^3], plain (x, y, z) order: 1 iff the block of 8^3 cells or one of its 26 neighbours holds a set bit."""
    assert H % B == 0
    G = H // B
    blocks = dense_of(bitfield, C, H).reshape(C, G, B, G, B, G, B).any(axis=(2, 4, 6))
    pad = np.zeros((C, G + 2, G + 2, G + 2), bool)
    pad[:, 1:-1, 1:-1, 1:-1] = blocks
    out = np.zeros_like(blocks)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out |= pad[:, dx:dx + G, dy:dy + G, dz:dz + G]
    return out.reshape(-1).astype(np.uint8)


# ------------------------------------------------------------------ the 64-point test
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _level(mx, C):
    return np.clip(np.frexp(mx.astype(F32))[1], 0, C - 1).astype(np.int64)


def step_constants(max_steps, C, H):
    dt_min = F32(F32(2 * F32(SQRT3)) / F32(max_steps))
    dt_max = F32(F32(2 * F32(SQRT3)) * F32(1 << (C - 1)) / F32(H))
    return dt_min, dt_max, min(dt_max, max(dt_min, F32(0)))  # dt_const = clamp(0, dt_min, dt_max)


def confine(mask, rays_o, rays_d, t0, fars, bound, C, H, max_steps):
    """-> (stated [N] bool, empty [N] bool, far2 [N] f32).  stated: the test makes a statement about the ray (the marcher's lattice
    walk would run, and the per-ray conditions hold); empty: no lattice point can be occupied; far2: the lowered far."""
    o, d = np.asarray(rays_o, F32).reshape(-1, 3), np.asarray(rays_d, F32).reshape(-1, 3)
    t0, far = np.asarray(t0, F32), np.asarray(fars, F32)
    N, G = o.shape[0], H // B
    bound = F32(bound)
    with np.errstate(all="ignore"):
        span = (far - t0).astype(F32)
        step = (span * F32(1.0 / 63.0)).astype(F32)
        dmax = np.abs(d).max(axis=1)
        delta = (F32(1.25) * (F32(0.5) * step * dmax) + bound * F32(1.0 / 1048576.0)).astype(F32)
        edge0 = F32(2 * B) * min(F32(1), bound) * F32(1.0 / H)
        stated = (t0 >= 0) & (t0 < far) & (span >= far * F32(1.0 / 1024.0)) & (span > F32(1e-6)) & (delta <= F32(0.9) * edge0)
        lane = np.arange(64, dtype=F32)[None, :]
        s = _fma(lane, step[:, None], t0[:, None])                                     # [N,64]
        p = np.clip(_fma(s[:, :, None], d[:, None, :], o[:, None, :]), -bound, bound)  # [N,64,3]
        p = np.where(np.isnan(p), -bound, p)
        mx = np.abs(p).max(axis=2)
        _, _, dt_const = step_constants(max_steps, C, H)
        lvl_dt = int(np.clip(np.frexp(F32(np.float64(dt_const * F32(H)) * 0.5))[1], 0, C - 1))
        lo = np.maximum(_level(np.maximum(mx - delta[:, None], 0), C), lvl_dt)
        hi = np.maximum(_level(mx + delta[:, None], C), lvl_dt)
        hit = np.zeros((N, 64), bool)
        for level in range(C):
            rb = F32(1) / min(F32(1 << level), bound)
            cell = np.clip(_fma(p, rb, F32(1)) * F32(0.5 * H), 0, H - 1).astype(np.int64) >> 3
            idx = level * G ** 3 + (cell[..., 0] * G + cell[..., 1]) * G + cell[..., 2]
            hit |= (lo <= level) & (level <= hi) & (mask[idx] != 0)
        empty = stated & ~hit.any(axis=1)
        last = 63 - np.argmax(hit[:, ::-1], axis=1)
        cut = _fma((last + 1).astype(F32), step, t0)
        far2 = np.where(stated & ~empty & (last < 63), np.minimum(far, cut), far).astype(F32)
    return stated, empty, far2


# ------------------------------------------------------------------ grids and rays
def _single_cells(H):
    ends = (0, H // 2 - 1, H - 1)  # low face, an interior coordinate right under a block boundary, high face
    out = []
    for x in ends:
        for y in ends:
            for z in ends:
                n_mid = (x == ends[1]) + (y == ends[1]) + (z == ends[1])
                if n_mid < 3:  # 8 corners, 12 edges, 6 faces
                    out.append((x, y, z))
    return out


def grids(C, H, seed=0):
    """name -> dense bool [C,H,H,H]."""
    rng = np.random.RandomState(seed)
    out = {}
    for pct in (1, 5, 50):
        out["random%d" % pct] = rng.rand(C, H, H, H) < pct / 100.0
    G = H // B
    out["blocky_aligned"] = np.repeat(np.repeat(np.repeat(rng.rand(C, G, G, G) < 0.05, B, 1), B, 2), B, 3)
    g = np.zeros((C, H, H, H), bool)
    for _ in range(12):  # boxes of odd sizes at odd offsets: straddle coarse-block boundaries
        c = rng.randint(C)
        lo = rng.randint(0, H - 13, 3)
        sz = rng.randint(1, 13, 3)
        g[c, lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = True
    out["blocky_odd"] = g
    out["empty"] = np.zeros((C, H, H, H), bool)
    out["full"] = np.ones((C, H, H, H), bool)
    for (x, y, z) in _single_cells(H):
        g = np.zeros((C, H, H, H), bool)
        g[:, x, y, z] = True
        out["cell_%d_%d_%d" % (x, y, z)] = g
    return out


def rays(N, bound, dense, seed=0):
    """N rays, float32: a quarter from outside towards random points of the volume, a quarter aimed at occupied cells of the last
    cascade (all of them, where nothing is occupied, at random points), a quarter nearly axis-parallel along the faces of coarse
    blocks (grazing), a quarter starting inside the volume."""
    rng = np.random.RandomState(seed)
    C, H = dense.shape[0], dense.shape[1]
    q = N // 4
    o, d = np.zeros((N, 3)), np.zeros((N, 3))

    def sphere(n, r):
        v = rng.randn(n, 3)
        return r * v / np.linalg.norm(v, axis=1, keepdims=True)
    # outside -> random targets
    o[:q] = sphere(q, rng.uniform(2.0, 4.0, (q, 1)) * bound)
    d[:q] = rng.uniform(-bound, bound, (q, 3)) - o[:q]
    # outside -> occupied cells (cell centre of the last cascade +- half a cell)
    occ = np.argwhere(dense[C - 1])
    o[q:2 * q] = sphere(q, rng.uniform(1.8, 4.0, (q, 1)) * bound)
    if len(occ):
        cells = occ[rng.randint(0, len(occ), q)] + rng.uniform(0, 1, (q, 3))
        tgt = (cells / H * 2 - 1) * bound
    else:
        tgt = rng.uniform(-bound, bound, (q, 3))
    d[q:2 * q] = tgt - o[q:2 * q]
    # grazing: travel along one axis inside (or a hair beside) a face shared by coarse blocks of some cascade
    G = H // B
    for i in range(2 * q, 3 * q):
        ax = rng.randint(3)
        mb = min(2.0 ** rng.randint(C), bound)
        pos = (rng.randint(0, G + 1, 3) / G * 2 - 1) * mb + rng.choice([0.0, 1e-7, -1e-7, 1e-4, -1e-4], 3)
        pos[ax] = -3.0 * bound * rng.choice([-1, 1])
        o[i] = pos
        dd = rng.choice([0.0, 1e-5, -1e-5, 1e-3], 3) + 1e-9
        dd[ax] = -np.sign(pos[ax])
        d[i] = dd
    # inside the volume
    o[3 * q:] = rng.uniform(-bound, bound, (N - 3 * q, 3))
    d[3 * q:] = rng.randn(N - 3 * q, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F32), d.astype(F32)
