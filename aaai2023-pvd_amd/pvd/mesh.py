"""A trained field as a triangle mesh, extracted on the device.

reference: extract_fields / extract_geometry, distill_mutual/utils.py:442-488 -- a density volume of resolution^3 samples filled
chunk by chunk through the host, mcubes.marching_cubes on the host, vertices mapped back into the box.  Here the volume is filled
on the device and the surface is extracted by the kernels of csrc/mesh.hip (include/pvd_hip_mesh.h: marching tetrahedra on the
Kuhn split; shared vertices, watertight, deterministic order); the two totals are the only values read back.  method="nets" takes
the kernels of csrc/mesh_nets.hip instead (csrc/pvd_hip_mesh_nets.h: naive surface nets, one vertex per active cell, two triangles per
crossing lattice edge -- fewer and better-shaped triangles, not manifold at ambiguous faces, open where it leaves the box).

The reference's meshes carry the density "floaters" of the field as small closed shells (network.py:601: "lots of noisy outliers
in hashnerf"); label_components / drop_components (csrc/components.hip, include/pvd_hip_components.h) take them out of the volume
on the device before it is meshed.
"""
import torch


def _box(bmin, bmax, device):
    lo = torch.as_tensor(bmin, dtype=torch.float32, device=device).reshape(3).contiguous()
    hi = torch.as_tensor(bmax, dtype=torch.float32, device=device).reshape(3).contiguous()
    return lo, hi


@torch.no_grad()
def density_field(query, R, bmin, bmax, chunk=1 << 21, device=None):
    """u [R,R,R] f32 on the device, x-major as extract_fields fills it (utils.py:442-470): u[i,j,k] = query(point (i,j,k) of the
    linspace^3 lattice of the box).  `query` maps [M,3] device points to M values, e.g. ``lambda x: model.density(x)["sigma"]``.
    The points are made on the device, `chunk` at a time; nothing is copied to the host.  bmin / bmax: 3 floats or tensors."""
    R = int(R)
    if R < 2:
        raise ValueError("R must be at least 2")
    if device is None:
        device = bmin.device if torch.is_tensor(bmin) else torch.device("cuda", torch.cuda.current_device())
    lo, hi = _box(bmin, bmax, device)
    # the lattice as the emit pass maps it back: lo + i / (R - 1) * (hi - lo)
    axes = torch.arange(R, dtype=torch.float32, device=device)[:, None] / float(R - 1) * (hi - lo)[None, :] + lo[None, :]  # [R,3]
    u = torch.empty(R, R, R, dtype=torch.float32, device=device)
    flat = u.view(-1)
    N = R ** 3
    for s in range(0, N, int(chunk)):
        n = torch.arange(s, min(s + int(chunk), N), dtype=torch.int64, device=device)
        pts = torch.stack([axes[n // (R * R), 0], axes[(n // R) % R, 1], axes[n % R, 2]], dim=1)
        flat[s:s + n.numel()] = query(pts).reshape(-1).to(torch.float32)
    return u


MESH_METHODS = ("tetrahedra", "nets")


def extract_mesh(field, thresh, bmin, bmax, with_normals=False, method="tetrahedra"):
    """(vertices [V,3] f32, triangles [T,3] int32), device tensors, of the surface field = thresh (inside: field > thresh; normals
    point outwards); field [R,R,R] f32 on the device, vertices in the box bmin .. bmax.  One read-back: the two totals.
    with_normals=True: (vertices, triangles, normals [V,3] f32) -- the outward unit normal of every vertex from the gradient of the
    field (include/pvd_hip_mesh_attr.h), one more launch on the same workspace; (0,0,0) where the gradient is zero or not finite.
    method="tetrahedra" (the default): marching tetrahedra on the Kuhn split (include/pvd_hip_mesh.h), watertight, vertices on lattice
    edges.  method="nets": naive surface nets (csrc/pvd_hip_mesh_nets.h) -- one vertex per active cell at the mean of its edge
    crossings, two triangles per crossing interior lattice edge; no slivers by construction and a fraction of the triangles, but four
    quads meet in one edge at an ambiguous lattice face (not manifold there), and the surface is open where it leaves the box.
    Anything else: ValueError."""
    import pvd_hip
    if method not in MESH_METHODS:
        raise ValueError("method must be one of %s, got %r" % (MESH_METHODS, method))
    if field.dim() != 3 or field.shape[0] != field.shape[1] or field.shape[0] != field.shape[2]:
        raise ValueError("field must be [R,R,R]")
    field = field.contiguous()
    R, dev = int(field.shape[0]), field.device
    lo, hi = _box(bmin, bmax, dev)
    if method == "nets":
        workspace_bytes, count, emit, emit_normals = (pvd_hip.mesh_nets_workspace_bytes, pvd_hip.mesh_nets_count, pvd_hip.mesh_nets_emit,
                                                      pvd_hip.mesh_nets_normals)
    else:
        workspace_bytes, count, emit, emit_normals = pvd_hip.mesh_workspace_bytes, pvd_hip.mesh_count, pvd_hip.mesh_emit, pvd_hip.mesh_normals
    ws = torch.empty(workspace_bytes(R), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    count(field, R, float(thresh), ws, totals)
    V, T = (int(v) for v in totals.tolist())
    vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
    triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
    emit(field, R, float(thresh), lo, hi, ws, vertices, triangles)
    if not with_normals:
        return vertices, triangles
    normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
    emit_normals(field, R, float(thresh), lo, hi, ws, normals)
    return vertices, triangles, normals


def _cube(field):
    if field.dim() != 3 or field.shape[0] != field.shape[1] or field.shape[0] != field.shape[2]:
        raise ValueError("field must be [R,R,R]")
    return field.contiguous(), int(field.shape[0])


def label_components(field, thresh):
    """(labels [R,R,R] int32, sizes [R,R,R] int32, stats) of the connected components of the set field > thresh, under the
    connectivity of the mesher's Kuhn split (14 neighbours).  labels: the smallest linear index of the point's component, -1
    outside; sizes: the component's number of points at its label, 0 elsewhere; both stay on the device.  stats, the one
    read-back: (components, inside points, size of the largest component, its label) as Python ints.
    The components follow the Kuhn split's connectivity whatever mesher is used afterwards: with extract_mesh(method="nets") the
    shells of the mesh can differ from them at ambiguous lattice faces."""
    import pvd_hip
    field, R = _cube(field)
    labels = torch.empty(R, R, R, dtype=torch.int32, device=field.device)
    sizes = torch.empty(R, R, R, dtype=torch.int32, device=field.device)
    stats = torch.zeros(4, dtype=torch.int32, device=field.device)
    pvd_hip.components_label(field, R, float(thresh), labels, sizes, stats)
    return labels, sizes, tuple(int(v) for v in stats.tolist())


def _drop(field, R, thresh, min_points, largest_only, out):
    """-> (stats, kept) as device tensors; out <- the filtered field"""
    import pvd_hip
    dev = field.device
    labels = torch.empty(R ** 3, dtype=torch.int32, device=dev)
    sizes = torch.empty(R ** 3, dtype=torch.int32, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    kept = torch.zeros(2, dtype=torch.int32, device=dev)
    pvd_hip.components_label(field, R, float(thresh), labels, sizes, stats)
    pvd_hip.components_filter(field, labels, sizes, stats, R, float(thresh), int(min_points), bool(largest_only), out, kept)
    return stats, kept


def drop_components(field, thresh, min_points=0, largest_only=False):
    """(field', kept): field with every point of a dropped component set to thresh, i.e. moved outside -- dropped are the components
    of fewer than min_points points and, with largest_only, all but the largest one (ties: the one with the smaller label).  The
    mesh of field' is the mesh of field without the shells of the dropped components, vertex bits included.  field is not changed.
    kept, the one read-back: (components kept, points kept).
    The components follow the Kuhn split's connectivity: with extract_mesh(method="nets") a dropped component's shell can differ from
    the shells of the mesh at ambiguous lattice faces (two components that touch across a face diagonal share a nets edge)."""
    field, R = _cube(field)
    out = torch.empty_like(field)
    _, kept = _drop(field, R, thresh, min_points, largest_only, out)
    return out, tuple(int(v) for v in kept.tolist())


def default_threshold(model):
    """min(density_thresh, mean_density) for a model with an occupancy grid -- the level its own marcher treats as empty
    (renderer.py: update_extra_state) --, density_thresh otherwise.  A mean_density of 0 is what a model carries whose grid was
    never updated (a student that marches on its teacher's grid): it says nothing, and density_thresh alone is used."""
    thresh = float(model.density_thresh)
    if getattr(model, "cuda_ray", False):
        mean = float(model.mean_density)
        if mean > 0.0:
            thresh = min(thresh, mean)
    return thresh


def extract_geometry(model, resolution=256, threshold=None, bmin=None, bmax=None, chunk=1 << 21, return_field=False, min_points=0,
                     largest_only=False, return_counts=False, method="tetrahedra"):
    """reference: extract_geometry, utils.py:473-488, with the density of `model` as the query.  The box defaults to
    model.aabb_infer, the threshold to default_threshold(model).  Returns (vertices, triangles) on the device (and the density
    volume with return_field=True).  min_points > 0 or largest_only: the volume is filtered in place by drop_components' rule
    between the two steps (the returned volume is the filtered one); return_counts=True then appends (components found,
    components kept, points kept), None where nothing was filtered.  method: extract_mesh's mesher, "tetrahedra" or "nets"."""
    if method not in MESH_METHODS:
        raise ValueError("method must be one of %s, got %r" % (MESH_METHODS, method))
    aabb = model.aabb_infer
    lo = aabb[:3] if bmin is None else bmin
    hi = aabb[3:] if bmax is None else bmax
    if threshold is None:
        threshold = default_threshold(model)
    u = density_field(lambda x: model.density(x)["sigma"], resolution, lo, hi, chunk=chunk, device=aabb.device)
    counts = None
    if int(min_points) > 0 or largest_only:
        stats, kept = _drop(u, int(resolution), threshold, min_points, largest_only, u)
        if return_counts:
            counts = (int(stats[0]),) + tuple(int(v) for v in kept.tolist())
    vertices, triangles = extract_mesh(u, threshold, lo, hi, method=method)
    result = (vertices, triangles, u) if return_field else (vertices, triangles)
    return result + (counts,) if return_counts else result


@torch.no_grad()
def vertex_colors(model, vertices, normals, chunk=1 << 20, autocast=True):
    """[V,3] f32 in [0,1] on the device: the colour head of `model` at every vertex, seen straight on -- rgb = model(x, d)[1] with
    d = -normal, `chunk` rows at a time, under fp16 autocast as evaluate_views renders (autocast=False: f32).  A vertex whose
    normal is (0,0,0) is looked at along (0,0,-1).  A vertex whose position or normal is not finite never reaches the model -- the
    centre of model.aabb_infer is evaluated in its place -- and gets the colour 0."""
    V = int(vertices.shape[0])
    out = torch.empty(V, 3, dtype=torch.float32, device=vertices.device)
    if V == 0:
        return out
    aabb = model.aabb_infer.to(device=vertices.device, dtype=torch.float32)
    centre = (aabb[:3] + aabb[3:]) * 0.5
    down = torch.tensor([0.0, 0.0, -1.0], device=vertices.device)
    for s in range(0, V, int(chunk)):
        x, n = vertices[s:s + int(chunk)].to(torch.float32), normals[s:s + int(chunk)].to(torch.float32)
        bad = ~(torch.isfinite(x).all(dim=1) & torch.isfinite(n).all(dim=1))
        flat = bad | (n == 0).all(dim=1)
        x = torch.where(bad[:, None], centre[None, :], x).contiguous()
        d = torch.where(flat[:, None], down[None, :], -n).contiguous()
        with torch.autocast("cuda", dtype=torch.float16, enabled=bool(autocast)):
            rgb = model(x, d)[1]
        out[s:s + x.shape[0]] = torch.where(bad[:, None], torch.zeros_like(x), rgb.to(torch.float32).clamp(0.0, 1.0))
    return out


def extract_surface(model, resolution=256, threshold=None, bmin=None, bmax=None, chunk=1 << 21, min_points=0, largest_only=False,
                    normals=True, colors=True, simplify=0, smooth=0, smooth_lambda=0.5, smooth_mu=-0.53, clean=False,
                    min_shell_triangles=0, largest_shell_only=False, texture=0, texture_sh=0, texture_density=0.0, method="tetrahedra"):
    """extract_geometry with what a viewer needs next to the geometry, as a dict: vertices, triangles, normals (extract_mesh's
    with_normals) and colors (vertex_colors), None where not asked for; field (the density volume, filtered where min_points > 0
    or largest_only), threshold, and counts = (components found, components kept, points kept), None where nothing was filtered.
    Colours are taken along the normals: colors=True with normals=False computes them and returns normals=None.
    simplify=G > 0: the mesh, with the normals and colours asked for, goes through simplify_mesh with G cells per axis over the
    extraction box; the dict then also holds vertex_map and full_counts = (vertices, triangles) before the simplification.
    smooth=N > 0: N iterations of smooth_mesh (weights smooth_lambda, smooth_mu) over the extraction box, after the colours -- which
    are evaluated at the unsmoothed vertices, on the level set -- and before the simplification; the normals asked for are then
    face_vertex_normals of the smoothed mesh, and the dict also holds smoothed = N.  smooth=0: the dict is what it was.
    clean=True: the mesh, with the normals and colours it has by then, goes through clean_mesh (min_shell_triangles,
    largest_shell_only) last, after the simplification; the dict then also holds topology = dict(before, after), triangle_map, and
    vertex_map -- clean_mesh's, composed with simplify_mesh's where both ran, so that it still maps the extracted vertices.
    clean=False: the dict is what it was.
    texture=S > 0: an atlas with S x S texels per pair of triangles is baked last (bake_texture: the model's colour head at the surface
    point of every texel, seen along the mesh's normals, or the face normals where none were asked for), on the final mesh -- after
    the smoothing, the simplification and the clean-up; the dict then also holds texture [Ht,Wt,3], uv [T,3,2] and texture_cell = S.
    texture=0: the dict is what it was.
    texture_sh=L > 0 with texture=S > 0: bake_sh_texture (L bands of spherical harmonics per texel, the colour as a function of the
    view) in place of the flat bake; the dict then holds texture [Ht,Wt,L*L,3], texture_degree = L and texture_diffuse [Ht,Wt,3], the
    view-independent part, next to uv and texture_cell.  texture_sh=0: the dict is what it was.
    texture_density=D > 0: the flat bake goes onto an area-adaptive atlas (adaptive_atlas: D texels per unit length, a cell edge per
    triangle, at most texture=S where given and 64 otherwise); texture_cell is then that atlas.  With texture_sh it raises ValueError.
    texture_density=0: the dict is what it was.
    method="nets": the geometry and the normals come from the surface nets mesher (extract_mesh's method); everything after it takes
    (vertices, triangles) and works on them unchanged.  min_points / largest_only still filter by the Kuhn split's components.
    method="tetrahedra": the dict is what it was."""
    if method not in MESH_METHODS:
        raise ValueError("method must be one of %s, got %r" % (MESH_METHODS, method))
    aabb = model.aabb_infer
    lo = aabb[:3] if bmin is None else bmin
    hi = aabb[3:] if bmax is None else bmax
    if threshold is None:
        threshold = default_threshold(model)
    u = density_field(lambda x: model.density(x)["sigma"], resolution, lo, hi, chunk=chunk, device=aabb.device)
    counts = None
    if int(min_points) > 0 or largest_only:
        stats, kept = _drop(u, int(resolution), threshold, min_points, largest_only, u)
        counts = (int(stats[0]),) + tuple(int(v) for v in kept.tolist())
    nrm = col = None
    if normals or colors:
        vertices, triangles, nrm = extract_mesh(u, threshold, lo, hi, with_normals=True, method=method)
        if colors:
            col = vertex_colors(model, vertices, nrm)
    else:
        vertices, triangles = extract_mesh(u, threshold, lo, hi, method=method)
    return _finish_surface(model, vertices, triangles, nrm, col, normals, lo, hi, dict(field=u, threshold=float(threshold), counts=counts),
                           smooth, smooth_lambda, smooth_mu, simplify, clean, min_shell_triangles, largest_shell_only, texture, texture_sh, texture_density)


def _finish_surface(model, vertices, triangles, nrm, col, normals, lo, hi, extra, smooth, smooth_lambda, smooth_mu, simplify, clean,
                    min_shell_triangles, largest_shell_only, texture, texture_sh, texture_density=0.0):
    """The tail extract_surface and extract_surface_tsdf share: smoothing, the dict (with `extra` after the four mesh entries), the
    simplification, the clean-up and the texture bake, in extract_surface's order and with its meaning."""
    if int(smooth) > 0:
        vertices = smooth_mesh(vertices, triangles, iterations=int(smooth), lam=smooth_lambda, mu=smooth_mu, bmin=lo, bmax=hi)
        if normals:
            nrm = face_vertex_normals(vertices, triangles)
    out = dict(vertices=vertices, triangles=triangles, normals=nrm if normals else None, colors=col, **extra)
    if int(smooth) > 0:
        out["smoothed"] = int(smooth)
    if int(simplify) > 0:
        small = simplify_mesh(vertices, triangles, int(simplify), bmin=lo, bmax=hi, normals=out["normals"], colors=col)
        out.update(small, full_counts=(int(vertices.shape[0]), int(triangles.shape[0])))
    if clean:
        first = out.get("vertex_map")
        done = clean_mesh(out["vertices"], out["triangles"], normals=out["normals"], colors=out["colors"],
                          min_shell_triangles=min_shell_triangles, largest_shell_only=largest_shell_only)
        vmap = done["vertex_map"]
        if first is not None:  # extracted vertex -> simplified vertex -> cleaned vertex
            vmap = torch.where(first >= 0, vmap[first.clamp(min=0).long()], torch.full_like(first, -1))
        out.update(vertices=done["vertices"], triangles=done["triangles"], normals=done["normals"], colors=done["colors"],
                   vertex_map=vmap, triangle_map=done["triangle_map"], topology=dict(before=done["before"], after=done["after"]))
    if float(texture_density) > 0.0:
        if int(texture_sh) > 0:
            raise ValueError("texture_sh needs a uniform atlas: texture_density (the adaptive atlas) is for flat textures only")
        atlas = adaptive_atlas(out["vertices"], out["triangles"], float(texture_density), max_cell=int(texture) if int(texture) > 0 else 64)
        baked = bake_texture(model, out["vertices"], out["triangles"], atlas, normals=out["normals"])
        out.update(texture=baked["texture"], uv=baked["uv"], texture_cell=atlas)
    elif int(texture) > 0 and int(texture_sh) > 0:
        baked = bake_sh_texture(model, out["vertices"], out["triangles"], int(texture), degree=int(texture_sh), normals=out["normals"])
        out.update(texture=baked["texture"], uv=baked["uv"], texture_cell=int(texture), texture_degree=int(texture_sh),
                   texture_diffuse=baked["diffuse"])
    elif int(texture) > 0:
        baked = bake_texture(model, out["vertices"], out["triangles"], int(texture), normals=out["normals"])
        out.update(texture=baked["texture"], uv=baked["uv"], texture_cell=int(texture))
    return out


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: float x y z per vertex, (uchar 3, int a b c) per face.  normals [V,3]: float nx ny nz after z;
    colors [V,3] in [0,1]: uchar red green blue after those, round(clamp(c, 0, 1) * 255)."""
    import numpy as np

    def host(a, dtype):
        return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dtype).reshape(-1, 3)
    v, t = host(vertices, "<f4"), host(triangles, "<i4")
    faces = np.empty(len(t), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"] = 3
    faces["v"] = t
    fields, props = [("p", "<f4", (3,))], "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields.append(("c", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    rows = np.empty(len(v), dtype=fields)  # packed: 12, 24, 15 or 27 bytes per vertex
    rows["p"] = v
    if normals is not None:
        rows["n"] = host(normals, "<f4")
    if colors is not None:
        c = host(colors, "<f4")
        with np.errstate(invalid="ignore"):
            rows["c"] = np.rint(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0).astype("u1")
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\nproperty list uchar int vertex_indices\n"
              "end_header\n" % (len(v), props, len(t)))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rows.tobytes())
        f.write(faces.tobytes())
    return path


def read_ply(path):
    """(vertices [V,3] f32, triangles [T,3] int32, normals [V,3] f32 | None, colors [V,3] f32 in [0,1] | None) of a file write_ply
    wrote, in any of its four vertex layouts, as host tensors; colours come back as byte / 255."""
    import numpy as np
    kinds = {"float": "<f4", "uchar": "u1"}
    with open(path, "rb") as f:
        if f.readline() != b"ply\n" or f.readline() != b"format binary_little_endian 1.0\n":
            raise ValueError("%s: not a binary little-endian PLY" % path)
        counts, fields, element = {}, [], None
        for line in iter(f.readline, b"end_header\n"):
            words = line.decode("ascii").split()
            if not words:
                raise ValueError("%s: the header does not end" % path)
            if words[0] == "element":
                element = words[1]
                counts[element] = int(words[2])
            elif words[0] == "property" and element == "vertex" and words[1] in kinds:
                fields.append((words[2], kinds[words[1]]))
            elif line != b"property list uchar int vertex_indices\n":
                raise ValueError("%s: unexpected header line %r" % (path, line))
        rows = np.frombuffer(f.read(np.dtype(fields).itemsize * counts["vertex"]), np.dtype(fields))
        faces = np.frombuffer(f.read(13 * counts["face"]), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    if len(rows) != counts["vertex"] or len(faces) != counts["face"] or not np.all(faces["n"] == 3):
        raise ValueError("%s: truncated, or a face that is not a triangle" % path)

    def columns(names, scale=None):
        if not all(n in rows.dtype.names for n in names):
            return None
        a = np.stack([rows[n] for n in names], axis=1).astype(np.float32)
        return torch.from_numpy(a / np.float32(scale) if scale else a)
    return (columns(("x", "y", "z")), torch.from_numpy(np.array(faces["v"], np.int32)), columns(("nx", "ny", "nz")),
            columns(("red", "green", "blue"), 255.0))


def default_grid(T):
    """Cells per axis mesh_distance uses for a mesh of T triangles: round(sqrt(T / 8)), clamped to 1 .. 256.  An extracted surface
    of T triangles crosses about T / 5 cells of its lattice (R ~ sqrt(T / 5) per axis), so this keeps a cell near 1.3 lattice
    spacings and rho near one cell: rings 0 .. 2 decide a query close to the surface.  profiles/mesh_dist.txt has the timings."""
    return max(1, min(256, int(round((max(int(T), 0) / 8.0) ** 0.5))))


def _finite_box(vertices):
    """Bounding box of the finite vertices, (lo, hi) f32 [3] on the device; the unit box where there is none."""
    ok = torch.isfinite(vertices).all(dim=1, keepdim=True)
    inf = torch.tensor(float("inf"), device=vertices.device)
    lo = torch.where(ok, vertices, inf).amin(dim=0) if vertices.shape[0] else inf.expand(3)
    hi = torch.where(ok, vertices, -inf).amax(dim=0) if vertices.shape[0] else -inf.expand(3)
    none = ~torch.isfinite(lo) | ~torch.isfinite(hi)
    return torch.where(none, torch.zeros_like(lo), lo).contiguous(), torch.where(none, torch.ones_like(hi), hi).contiguous()


def mesh_distance(points, vertices, triangles, max_dist, bmin=None, bmax=None, grid=None):
    """(dist [N] f32, tri [N] int32), device tensors: the distance from every row of points [N,3] to the mesh (vertices [V,3] f32,
    triangles [T,3] int32) and the index of the nearest triangle, exact in float64 and rounded once (include/pvd_hip_mesh_dist.h;
    csrc/mesh_dist.hip).  (max_dist, -1) where nothing is nearer than max_dist (finite, > 0) -- max_dist bounds the work per point --
    and (NaN, -1) for a point that is not finite.  Triangles with an index outside [0, V) or a corner that is not finite are
    ignored.  The grid of grid^3 cells (default: default_grid(T)) lies over bmin .. bmax (default: the bounding box of the finite
    vertices); neither changes a bit of the result, only the time."""
    import pvd_hip
    dev = vertices.device
    points = points.to(torch.float32).reshape(-1, 3).contiguous()
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    T = int(triangles.shape[0])
    G = default_grid(T) if grid is None else max(1, min(pvd_hip.MESH_DIST_MAX_G, int(grid)))
    box = _finite_box(vertices) if bmin is None or bmax is None else None
    lo = box[0] if bmin is None else _box(bmin, bmin, dev)[0]
    hi = box[1] if bmax is None else _box(bmax, bmax, dev)[0]
    ws = torch.empty(pvd_hip.mesh_dist_workspace_bytes(T, G), dtype=torch.uint8, device=dev)
    pvd_hip.mesh_dist_build(vertices, triangles, lo, hi, G, ws)
    dist = torch.empty(points.shape[0], dtype=torch.float32, device=dev)
    tri = torch.empty(points.shape[0], dtype=torch.int32, device=dev)
    pvd_hip.mesh_dist_query(points, T, G, ws, float(max_dist), dist, tri)
    return dist, tri


def sample_surface(vertices, triangles, n, seed):
    """points [n,3] f32 on the device, uniform over the surface: a triangle is drawn with probability proportional to its area
    (cumulative sum + searchsorted), a point in it by square-root barycentrics; a seeded device generator, so the same seed gives
    the same bits.  Invalid triangles and triangles of area 0 get no samples; a mesh without area gives an empty tensor."""
    dev = vertices.device
    v, t = vertices.to(torch.float32).reshape(-1, 3), triangles.to(torch.int64).reshape(-1, 3)
    if v.shape[0] == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=dev)
    ok = ((t >= 0) & (t < v.shape[0])).all(dim=1)
    corners = v[torch.where(ok[:, None], t, torch.zeros_like(t))].to(torch.float64)  # [T,3,3]
    ok &= torch.isfinite(corners).all(dim=2).all(dim=1)
    area = torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]).norm(dim=1) * 0.5
    area = torch.where(ok & torch.isfinite(area), area, torch.zeros_like(area))
    cum = torch.cumsum(area, dim=0)
    if int(n) <= 0 or cum.numel() == 0 or not float(cum[-1]) > 0.0:
        return torch.empty(0, 3, dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    u = torch.rand(int(n), 3, dtype=torch.float64, device=dev, generator=gen)
    # the first triangle whose cumulative area exceeds the draw: never one of area 0 (its cumulative value equals its predecessor's)
    pick = torch.searchsorted(cum, u[:, 0] * cum[-1], right=True).clamp(max=cum.numel() - 1)
    pick = torch.where(area[pick] > 0, pick, torch.argmax(area).expand_as(pick))  # (a draw of exactly the total)
    s = torch.sqrt(u[:, 1])
    w = torch.stack([1.0 - s, s * (1.0 - u[:, 2]), s * u[:, 2]], dim=1)  # [n,3]
    return (w[:, :, None] * corners[pick]).sum(dim=1).to(torch.float32)


def compare_meshes(va, ta, vb, tb, tau, max_dist=None, samples=0, seed=0, volume=0):
    """How far apart two meshes are, as a dict.  The points of a mesh are its vertices, or `samples` surface samples
    (sample_surface; seeds `seed` for A and `seed + 1` for B) when samples > 0; every point of A is measured against mesh B and
    the other way round (mesh_distance; max_dist defaults to the diagonal of the joint bounding box).
        a_to_b, b_to_a   mean distance from A's points to B, from B's points to A
        chamfer          their sum
        hausdorff        the larger of the two largest distances
        precision        share of A's points within tau of B;  recall: the same for B's points;  fscore: their harmonic mean
        n_a, n_b         points measured;  saturated_a, saturated_b: those with no triangle within max_dist (or not finite)
    Saturated rows count as max_dist in the means and the maxima and never as within tau; rows that are not finite are left out
    of the means, the maxima and the shares' denominators.  The
    reductions run in float64 on the device and come back in one read-back (the default max_dist costs one more).
    volume=R > 0 adds a volume overlap: both meshes are voxelised (voxelize_mesh) on one R^3 lattice over the joint bounding box, and
        iou                  points inside both / points inside either (0.0 where neither has any)
        volume_a, volume_b   points inside x the volume of a lattice cell
        leaky_a, leaky_b     columns of the lattice that saw the mesh open or inconsistently oriented (voxelize_mesh); not 0: the
                             mesh has no inside there, and the three figures above mean little
    join the dict."""
    dev = va.device
    va, vb = va.to(torch.float32).reshape(-1, 3), vb.to(torch.float32).reshape(-1, 3)
    if max_dist is None:
        lo_a, hi_a = _finite_box(va)
        lo_b, hi_b = _finite_box(vb)
        diag = float((torch.maximum(hi_a, hi_b) - torch.minimum(lo_a, lo_b)).to(torch.float64).norm())
        max_dist = diag if diag > 0.0 else 1.0
    pa = sample_surface(va, ta, samples, seed) if int(samples) > 0 else va
    pb = sample_surface(vb, tb, samples, int(seed) + 1) if int(samples) > 0 else vb

    def one_side(points, v, t):
        d, tri = mesh_distance(points, v, t, max_dist)
        d = d.to(torch.float64)
        ok = torch.isfinite(d)
        n = ok.sum().to(torch.float64).clamp(min=1.0)
        dz = torch.where(ok, d, torch.zeros_like(d))
        return torch.stack([dz.sum() / n, dz.max() if d.numel() else dz.sum(), ((d <= float(tau)) & (tri >= 0)).sum() / n,
                            (tri < 0).sum().to(torch.float64)])
    both = torch.cat([one_side(pa, vb, tb), one_side(pb, va, ta)]).tolist()
    (m_ab, h_ab, prec, sat_a), (m_ba, h_ba, rec, sat_b) = both[:4], both[4:]
    out = dict(a_to_b=m_ab, b_to_a=m_ba, chamfer=m_ab + m_ba, hausdorff=max(h_ab, h_ba), precision=prec, recall=rec,
               fscore=2.0 * prec * rec / (prec + rec) if prec + rec > 0.0 else 0.0, n_a=int(pa.shape[0]), n_b=int(pb.shape[0]),
               saturated_a=int(sat_a), saturated_b=int(sat_b))
    if int(volume) > 0:
        out.update(_volume_overlap(va, ta, vb, tb, volume))
    return out


def simplify_mesh(vertices, triangles, grid, bmin=None, bmax=None, normals=None, colors=None):
    """The mesh made smaller by vertex clustering on a grid of grid^3 cells (1 .. 512 per axis) over the box bmin .. bmax (default: the
    bounding box of the finite vertices; vertices outside a given box are projected onto it), as a dict of device tensors: vertices
    [V',3] f32 -- one per cell that a surviving triangle touches, the mean of the cell's vertices --, triangles [T',3] int32 -- those
    whose corners lie in three different cells, in input order and orientation --, normals and colors (None where not given) -- the
    cell means, normals renormalised ((0,0,0) where the mean is zero or not finite), colours clamped to [0,1] --, and vertex_map [V]
    int32, the new index of every input vertex (-1: not finite, or in a cell no surviving triangle touches).  Every sum is an integer
    sum: the result is bit-identical from run to run (include/pvd_hip_mesh_simplify.h; csrc/mesh_simplify.hip).  Duplicate output
    triangles are not merged and the result is not guaranteed manifold: clean_mesh cancels the collapsed sheets those duplicates are.  No vertex that keeps an index moves further than one cell
    (plus rounding) per axis.  One read-back: the two totals."""
    import pvd_hip
    dev = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    V, T, G = int(vertices.shape[0]), int(triangles.shape[0]), int(grid)
    parts = [a.to(torch.float32).reshape(V, 3) for a in (normals, colors) if a is not None]
    attrs = torch.cat(parts, dim=1).contiguous() if parts else None
    K = 3 * len(parts)
    box = _finite_box(vertices) if bmin is None or bmax is None else None
    lo = box[0] if bmin is None else _box(bmin, bmin, dev)[0]
    hi = box[1] if bmax is None else _box(bmax, bmax, dev)[0]
    ws = torch.empty(pvd_hip.mesh_simplify_workspace_bytes(V, T, G, K), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    pvd_hip.mesh_simplify_count(vertices, triangles, lo, hi, G, K, ws, totals)
    Vn, Tn = (int(v) for v in totals.tolist())
    out_v = torch.empty(Vn, 3, dtype=torch.float32, device=dev)
    out_t = torch.empty(Tn, 3, dtype=torch.int32, device=dev)
    out_a = torch.empty(Vn, K, dtype=torch.float32, device=dev) if K else None
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    pvd_hip.mesh_simplify_emit(vertices, triangles, attrs, lo, hi, G, ws, out_v, out_a, out_t, vmap)
    nrm = col = None
    if normals is not None:
        mean = out_a[:, :3]
        length = torch.linalg.norm(mean, dim=1, keepdim=True)
        ok = torch.isfinite(length) & (length > 0)
        nrm = torch.where(ok, mean / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(mean)).contiguous()
    if colors is not None:
        col = out_a[:, K - 3:].clamp(0.0, 1.0).contiguous()
    return dict(vertices=out_v, triangles=out_t, normals=nrm, colors=col, vertex_map=vmap)


def smooth_mesh(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, bmin=None, bmax=None, pinned=None, return_totals=False):
    """[V,3] f32 on the device: the vertices after `iterations` iterations of Taubin's lambda|mu filter -- a Laplacian pass with weight
    lam > 0, then one with weight mu < -lam, which takes out the noise at the scale of an edge without the shrinkage of plain Laplacian
    smoothing (mu=0 gives that).  Weighting: a pass moves every vertex by its weight towards the mean of the other corners of its
    triangles, so a neighbour counts once per triangle shared with it -- the uniform umbrella on a closed manifold mesh, half weight
    across a boundary edge.  Vertices of no valid triangle, vertices that are not finite and those with a non-zero byte in pinned [V]
    keep their input bits; triangles with an index outside [0, V), a corner that is not finite or a repeated index are ignored.  The
    topology and the triangle order are untouched: the triangles go with the result as they are.  The positions live on a 2^30
    lattice of the box bmin .. bmax (default: the bounding box of the finite vertices; vertices outside a given box are projected onto
    it) and every sum is an integer sum: the result is bit-identical from run to run (include/pvd_hip_mesh_smooth.h;
    csrc/mesh_smooth.hip).  iterations <= 0 returns a copy without a launch.  No read-back; return_totals=True returns (vertices,
    totals) with totals int64 [2] on the device: (row entries, largest row)."""
    import pvd_hip
    dev = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    if int(iterations) <= 0 or V == 0:
        return (vertices.clone(), totals) if return_totals else vertices.clone()
    box = _finite_box(vertices) if bmin is None or bmax is None else None
    lo = box[0] if bmin is None else _box(bmin, bmin, dev)[0]
    hi = box[1] if bmax is None else _box(bmax, bmax, dev)[0]
    if pinned is not None:
        pinned = (pinned.reshape(-1) != 0).to(torch.uint8).contiguous()
    ws = torch.empty(pvd_hip.mesh_smooth_workspace_bytes(V, T), dtype=torch.uint8, device=dev)
    pvd_hip.mesh_smooth_build(vertices, triangles, lo, hi, pinned, ws, totals)
    out = torch.empty_like(vertices)
    pvd_hip.mesh_smooth_run(vertices, T, lo, hi, ws, float(lam), float(mu), int(iterations), out)
    return (out, totals) if return_totals else out


def _topology_dict(totals):
    import pvd_hip
    d = {k: int(x) for k, x in zip(pvd_hip.MESH_TOPO_TOTALS, totals)}
    d["euler"] = d["referenced"] - d["edges"] + d["survivors"]
    d["closed"] = d["unbalanced"] == 0
    d["manifold"] = not (d["boundary"] or d["inconsistent"] or d["non_manifold"] or d["duplicate"] or d["cancelled"])
    return d


def _topo_build(vertices, triangles, with_flags):
    """(vertices, triangles as the kernels take them, workspace, totals [16] int64 on the device, tri_flags, vertex_shell)."""
    import pvd_hip
    dev = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    ws = torch.empty(pvd_hip.mesh_topo_workspace_bytes(V, T), dtype=torch.uint8, device=dev)
    totals = torch.empty(16, dtype=torch.int64, device=dev)
    flags = torch.empty(T, dtype=torch.uint8, device=dev) if with_flags else None
    shell = torch.empty(V, dtype=torch.int32, device=dev) if with_flags else None
    pvd_hip.mesh_topo_build(vertices, triangles, ws, totals, flags, shell)
    return vertices, triangles, ws, totals, flags, shell


def mesh_topology(vertices, triangles, return_flags=False):
    """Whether the mesh is a valid surface, as a dict of Python ints (include/pvd_hip_mesh_topo.h; csrc/mesh_topo.hip): valid and
    invalid triangles (an index outside [0, V), a corner that is not finite, a repeated index); duplicate and cancelled ones (the
    valid triangles on one vertex set keep one survivor in the orientation of their majority, or none when the two orientations
    balance); survivors; referenced (vertices a survivor uses); edges of the survivors and how many of them are boundary (one
    triangle), inconsistent (two triangles that traverse it in the same direction), non_manifold (three or more) and unbalanced
    (traversed forwards and backwards a different number of times); shells (connected sets of survivors), largest_size and
    largest_label (the smallest vertex index of the largest shell, -1 without one).  Then euler = referenced - edges + survivors,
    closed (unbalanced == 0) and manifold (no boundary, inconsistent, non-manifold edge, no duplicate, no cancelled triangle).
    return_flags=True adds the device tensors tri_flags [T] uint8 (bit0 invalid, bit1 duplicate, bit2 cancelled, bit3 / bit4 / bit5: a
    survivor with a boundary / inconsistent / non-manifold edge) and vertex_shell [V] int32 (the shell's label, -1: not referenced).
    Every figure is an integer that does not depend on any order: bit-identical from run to run.  One read-back: the totals."""
    _, _, _, totals, flags, shell = _topo_build(vertices, triangles, return_flags)
    out = _topology_dict(totals.tolist())
    if return_flags:
        out.update(tri_flags=flags, vertex_shell=shell)
    return out


def clean_mesh(vertices, triangles, normals=None, colors=None, min_shell_triangles=0, largest_shell_only=False):
    """The mesh without what makes it an invalid surface, as a dict of device tensors: triangles [T',3] int32 -- the survivors of
    mesh_topology (invalid and duplicate triangles dropped, collapsed sheets cancelled: the duplicates simplify_mesh leaves are
    exactly those) whose shell has at least min_shell_triangles survivors and, with largest_shell_only, is the largest one, in input
    order and corner order --, vertices [V',3] f32 -- the vertices those triangles use, in input order, bits copied --, normals and
    colors (None where not given) gathered by the same selection, vertex_map [V] and triangle_map [T] int32 (the new index, -1:
    dropped), and before / after, the mesh_topology dicts of the input and of the result.  Nothing is re-oriented, no hole is filled,
    no vertex is split or merged.  Cleaning twice changes nothing.  Two read-backs (before's totals, the two counts); after comes
    from a second build on the result, which costs what mesh_topology costs on it, one more read-back included."""
    import pvd_hip
    dev = vertices.device
    vertices, triangles, ws, totals, _, _ = _topo_build(vertices, triangles, False)
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    before = _topology_dict(totals.tolist())
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    pvd_hip.mesh_topo_clean_count(V, T, ws, int(min_shell_triangles), bool(largest_shell_only), counts)
    Vn, Tn = (int(x) for x in counts.tolist())
    out_v = torch.empty(Vn, 3, dtype=torch.float32, device=dev)
    out_t = torch.empty(Tn, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    tmap = torch.empty(T, dtype=torch.int32, device=dev)
    pvd_hip.mesh_topo_clean_emit(vertices, triangles, ws, out_v, out_t, vmap, tmap)
    slot = torch.where(vmap >= 0, vmap, torch.full_like(vmap, Vn)).long()  # the dropped vertices all go to one row behind the end

    def gathered(a):  # by vertex_map, without the read-back a boolean mask would make
        if a is None:
            return None
        a = a.reshape(V, -1)
        return torch.empty(Vn + 1, a.shape[1], dtype=a.dtype, device=dev).index_copy_(0, slot, a)[:Vn].contiguous()
    nrm, col = gathered(normals), gathered(colors)
    return dict(vertices=out_v, triangles=out_t, normals=nrm, colors=col, vertex_map=vmap, triangle_map=tmap, before=before,
                after=mesh_topology(out_v, out_t))


def face_vertex_normals(vertices, triangles):
    """[V,3] f32 unit normals from the faces: the sum of the area-weighted normals (half the cross products) of a vertex's triangles,
    renormalised; (0,0,0) where the sum is null or not finite.  Plain torch (index_add_ of floats): NOT bit-reproducible from run to
    run.  For meshes whose vertices were moved (smooth_mesh): the density-gradient normals of extract_mesh belong to the positions on
    the level set.  Triangles with an index outside [0, V) are ignored."""
    v = vertices.to(torch.float32).reshape(-1, 3)
    t = triangles.to(torch.int64).reshape(-1, 3)
    V = int(v.shape[0])
    acc = torch.zeros(V, 3, dtype=torch.float32, device=v.device)
    if V == 0 or int(t.shape[0]) == 0:
        return acc
    ok = ((t >= 0) & (t < V)).all(dim=1)
    t = t[ok]
    c = v[t]  # [T,3,3]
    face = torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]) * 0.5
    face = torch.where(torch.isfinite(face).all(dim=1, keepdim=True), face, torch.zeros_like(face))
    for k in range(3):
        acc.index_add_(0, t[:, k], face)
    length = torch.linalg.norm(acc, dim=1, keepdim=True)
    good = torch.isfinite(length) & (length > 0)
    return torch.where(good, acc / torch.where(good, length, torch.ones_like(length)), torch.zeros_like(acc)).contiguous()


def _tri_grid(api, vertices, triangles, bmin, bmax, grid):
    """(T, G, pairs, workspace): the uniform grid of csrc/mesh_tri_grid.h over the mesh, as the queries of `api` read it -- "mesh_ray":
    include/pvd_hip_mesh_ray.h, G^3 cells; "mesh_winding": include/pvd_hip_mesh_winding.h, G^2 cells over x and y.  One read-back: the
    two totals of the count pass."""
    import pvd_hip
    dev = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    T = int(triangles.shape[0])
    G = default_grid(T) if grid is None else int(grid)  # (a grid outside the binding's 1 .. MAX_G is its error, not clamped)
    lo, hi = _finite_box(vertices) if bmin is None or bmax is None else (None, None)
    if bmin is not None:
        lo = torch.as_tensor(bmin, dtype=torch.float32, device=dev).reshape(3).contiguous()
    if bmax is not None:
        hi = torch.as_tensor(bmax, dtype=torch.float32, device=dev).reshape(3).contiguous()
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    getattr(pvd_hip, api + "_count")(vertices, triangles, lo, hi, G, totals)
    pairs = int(totals.tolist()[0])
    ws = torch.empty(getattr(pvd_hip, api + "_workspace_bytes")(T, G, pairs), dtype=torch.uint8, device=dev)
    getattr(pvd_hip, api + "_build")(vertices, triangles, lo, hi, G, pairs, ws)
    return T, G, pairs, ws


def _ray_grid(vertices, triangles, bmin, bmax, grid):
    """The grid pvd_mesh_ray_cast and pvd_mesh_expose read."""
    return _tri_grid("mesh_ray", vertices, triangles, bmin, bmax, grid)


def mesh_raycast(origins, dirs, vertices, triangles, t_min=0.0, t_max=float("inf"), bmin=None, bmax=None, grid=None):
    """(t [N] f32, tri [N] int32, bary [N,2] f32), device tensors: the first hit of every ray (origins [N,3], dirs [N,3]; dirs need not
    be unit length, t is in units of |dir|) on the mesh (vertices [V,3] f32, triangles [T,3] int32) with t_min <= t < t_max -- the
    watertight test in unfused float64, rounded once (include/pvd_hip_mesh_ray.h; csrc/mesh_ray.hip).  tri is the triangle, bary the
    weights of its second and third corner.  (t_max, -1, (0, 0)) where nothing is hit, (NaN, -1, (0, 0)) for a ray that is not finite
    or has a zero direction.  Triangles with an index outside [0, V) or a corner that is not finite are ignored.  The grid of grid^3
    cells (default: default_grid(T); 1 .. 256, anything else raises) lies over bmin .. bmax (default: the bounding box of the finite
    vertices); neither changes a bit of the result, only the time -- but for the edge-on case include/pvd_hip_mesh_ray.h names.  One
    read-back: the two totals of the count pass."""
    import pvd_hip
    dev = vertices.device
    origins = origins.to(torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(torch.float32).reshape(-1, 3).contiguous()
    T, G, pairs, ws = _ray_grid(vertices, triangles, bmin, bmax, grid)
    N = int(origins.shape[0])
    t = torch.empty(N, dtype=torch.float32, device=dev)
    tri = torch.empty(N, dtype=torch.int32, device=dev)
    bary = torch.empty(N, 2, dtype=torch.float32, device=dev)
    pvd_hip.mesh_ray_cast(origins, dirs, T, G, pairs, ws, float(t_min), float(t_max), t, tri, bary)
    return t, tri, bary


# ------------------------------------------------------------------------------------------------ exposure: what a view can see
def exposure_directions(D=64):
    """[D,3] f32 (a host tensor): the default directions of mesh_exposure, a Fibonacci sphere -- z_i = 1 - (2 i + 1) / D, the azimuth
    (i + 1/2) pi (3 - sqrt 5), made in float64 and rounded to float32.  The same D gives the same directions; none of the default 64 has
    a zero component, so none runs along an axis or in a lattice plane of an extracted mesh."""
    import numpy as np
    i = np.arange(int(D), dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / float(D)
    r = np.sqrt(1.0 - z * z)
    phi = (i + 0.5) * (np.pi * (3.0 - np.sqrt(5.0)))
    return torch.from_numpy(np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32))


def mesh_exposure(vertices, triangles, dirs=None, samples=1, bmin=None, bmax=None, grid=None, band=None, return_totals=False):
    """counts [T,4] int32 on the device: per triangle the front rays cast, the front rays that escaped, the back rays cast and the back rays
    that escaped -- rays from `samples` points of the triangle (1: the centroid; 4: and three points towards the corners) along every
    direction of dirs [D,3] (D 1 .. 1024; default exposure_directions(64)); a ray is a front ray where it leaves on the side the
    triangle's winding faces (the outside of an extract_mesh surface), and it escapes when it meets no other valid triangle: an any-hit
    walk over mesh_raycast's grid with its watertight test (csrc/pvd_hip_mesh_expose.h has the definition to the operation;
    csrc/mesh_expose.hip).  A triangle with an index outside [0, V) or a corner that is not finite has four zeros.  Integers: identical
    from run to run, and independent of grid, the box and band (the triangles per launch; default: all in one) -- but for the edge-on
    case include/pvd_hip_mesh_ray.h names.  return_totals=True: (counts, dict of rays_cast, rays_escaped, front_exposed, back_exposed and
    hidden -- valid triangles with a front escape, with a back escape, with none), one more read-back.  See cull_hidden."""
    import pvd_hip
    dev = vertices.device
    T, G, pairs, ws = _ray_grid(vertices, triangles, bmin, bmax, grid)
    dirs = (exposure_directions(64) if dirs is None else dirs).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    counts = torch.empty(T, 4, dtype=torch.int32, device=dev)
    totals = torch.zeros(5, dtype=torch.int64, device=dev)
    step = T if band is None else int(band)
    if band is not None and step < 1:
        raise ValueError("band must be at least 1, got %d" % step)
    for s in range(0, T, max(step, 1)):
        e = min(s + step, T)
        pvd_hip.mesh_expose(dirs, int(samples), s, e, T, G, pairs, ws, counts[s:e], totals)
    if T == 0:  # nothing to launch: the arguments are still checked
        pvd_hip.mesh_expose(dirs, int(samples), 0, 0, T, G, pairs, ws, counts, totals)
    if not return_totals:
        return counts
    return counts, dict(zip(pvd_hip.MESH_EXPOSE_TOTALS, (int(x) for x in totals.tolist())))


def cull_hidden(vertices, triangles, normals=None, colors=None, mode="shells", sides="front", min_escaped=1, dirs=None, samples=1,
                grid=None, band=None):
    """The mesh without the geometry no outside view can see, as a dict shaped like clean_mesh's: vertices [V',3] f32 and triangles [T',3]
    int32 (what is kept, in input order, bits copied), normals and colors (None where not given) by the same selection, vertex_map [V]
    and triangle_map [T] int32 (the new index, -1: dropped), counts [T,4] (mesh_exposure's, of the input) and report: triangles_before /
    _after, vertices_before / _after, hidden_triangles (the valid triangles that are not exposed -- in mode="shells" that counts the
    unexposed triangles of a shell that is kept too, so it is NOT triangles_before - triangles_after there), shells_before, shells_dropped
    and totals (mesh_exposure's).  A triangle is EXPOSED when at least min_escaped of its front rays escape (sides="front": the orientation is
    trusted, as extract_mesh gives it) or of its front or of its back rays (sides="either": for meshes of unknown orientation).
    mode="shells" (default): a shell -- mesh_topology's vertex_shell -- is dropped only when none of its triangles is exposed, so a closed
    mesh stays closed and mesh_winding, voxelize_mesh and mesh_to_sdf still work on the result: cavity walls and enclosed blobs go, a part
    that is seen anywhere stays whole.  mode="triangles": every triangle that is not exposed is dropped; THIS OPENS THE SURFACE (the
    result has boundary edges wherever a visible part continues out of sight).  Triangles with an index outside [0, V) or a corner that is
    not finite are always dropped; a valid triangle whose first corner has no shell (a cancelled sheet) is judged on its own.  Vertices
    no kept triangle uses are dropped.  The selection is plain torch (an integer amax scatter per shell, masks, cumulative sums); the
    rays are the kernel's.  grid and band are mesh_exposure's: band triangles per launch (default: one launch for the whole mesh, several
    hundred milliseconds for a 256^3 extraction at 64 directions); the box is always the bounding box of the finite vertices."""
    if mode not in ("shells", "triangles") or sides not in ("front", "either"):
        raise ValueError("mode must be 'shells' or 'triangles' and sides 'front' or 'either', got %r and %r" % (mode, sides))
    dev = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    counts, totals = mesh_exposure(vertices, triangles, dirs, samples, grid=grid, band=band, return_totals=True)
    escaped = counts[:, 1] if sides == "front" else torch.maximum(counts[:, 1], counts[:, 3])
    exposed = escaped >= max(int(min_escaped), 1)
    topo = mesh_topology(vertices, triangles, return_flags=True)
    tl = triangles.long()
    in_range = ((tl >= 0) & (tl < V)).all(dim=1)
    safe = torch.where(in_range[:, None], tl, torch.zeros_like(tl))
    valid = in_range & (torch.isfinite(vertices[safe].reshape(T, 9)).all(dim=1) if V else in_range)
    label = torch.where(valid, topo["vertex_shell"].long()[safe[:, 0]], torch.full((T,), -1, dtype=torch.int64, device=dev)) if V else \
        torch.full((T,), -1, dtype=torch.int64, device=dev)
    slot = torch.where(label >= 0, label, torch.full_like(label, V))  # the triangles without a shell all go to one slot behind the end
    seen = torch.zeros(V + 1, dtype=torch.int32, device=dev).scatter_reduce_(0, slot, exposed.to(torch.int32), "amax")
    present = torch.zeros(V + 1, dtype=torch.int32, device=dev).scatter_reduce_(0, slot, valid.to(torch.int32), "amax")
    if mode == "shells":
        keep = valid & torch.where(label >= 0, seen[slot] > 0, exposed)
    else:
        keep = valid & exposed
    tmap = torch.where(keep, torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32) - 1, torch.full((T,), -1, dtype=torch.int32, device=dev))
    kept = tl[keep]
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[kept.reshape(-1)] = True
    vmap = torch.where(used, torch.cumsum(used.to(torch.int32), 0, dtype=torch.int32) - 1, torch.full((V,), -1, dtype=torch.int32, device=dev))
    out_t = vmap[kept].to(torch.int32).reshape(-1, 3).contiguous()
    out_v = vertices[used].contiguous()

    def gathered(a):
        return None if a is None else a.reshape(V, -1)[used].contiguous()
    figures = torch.stack([(valid & ~exposed).sum(), ((present[:V] > 0) & (seen[:V] == 0)).sum()]).tolist()
    report = dict(triangles_before=T, triangles_after=int(out_t.shape[0]), vertices_before=V, vertices_after=int(out_v.shape[0]),
                  hidden_triangles=int(figures[0]), shells_before=topo["shells"], shells_dropped=int(figures[1]), totals=totals)
    return dict(vertices=out_v, triangles=out_t, normals=gathered(normals), colors=gathered(colors), vertex_map=vmap, triangle_map=tmap,
                counts=counts, report=report)


def render_mesh(vertices, triangles, pose, intrinsics, H, W, normals=None, colors=None, bg_color=1.0, grid=None, texture=None,
                texture_cell=None):
    """The mesh seen from the camera `pose` ([4,4] cam2world; rays from pvd.scene.get_rays, unit directions, so t is a distance), as
    a dict of device tensors:
        depth [H,W] f32     the distance to the first hit, 0 where nothing is hit
        mask  [H,W] bool    hit or not;   tri [H,W] int32, bary [H,W,2] f32: mesh_raycast's
        normal [H,W,3]      the barycentric mean of the vertex normals [V,3], renormalised, where they are given; otherwise the unit
                            face normal turned towards the camera; (0,0,0) off the mesh (and where the mean or the face is null)
        color [H,W,3]       the barycentric mean of the vertex colours [V,3] over bg_color (a float or 3 floats); None without colors
    The interpolation is plain torch gathers on the cast's output.
    texture [Ht,Wt,3] with texture_cell = S (bake_texture's, for these triangles): color is sample_texture's bilinear lookup of the
    atlas at the hits instead (csrc/mesh_tex.hip), whatever colors holds.  A 4-D texture [Ht,Wt,K,3] (bake_sh_texture's) is an SH atlas:
    color is sample_sh_texture's, evaluated at each ray's direction (csrc/mesh_shtex.hip); K gives the number of bands.
    texture_cell = adaptive_atlas's dict (bake_texture returns it as texture_cell): the flat lookup on that atlas (csrc/mesh_atex.hip)."""
    from .scene import get_rays
    dev = vertices.device
    pose = torch.as_tensor(pose, dtype=torch.float32, device=dev).reshape(4, 4)
    r = get_rays(pose[None], intrinsics, int(H), int(W), -1)
    o, d = r["rays_o"].reshape(-1, 3).contiguous(), r["rays_d"].reshape(-1, 3).contiguous()
    t, tri, bary = mesh_raycast(o, d, vertices, triangles, grid=grid)
    mask = tri >= 0
    if int(triangles.shape[0]) == 0 or int(vertices.shape[0]) == 0:  # nothing to gather from: every pixel is background
        col = None
        if colors is not None or texture is not None:
            col = torch.as_tensor(bg_color, dtype=torch.float32, device=dev).expand(H, W, 3).contiguous()
        return dict(depth=torch.zeros(H, W, dtype=torch.float32, device=dev), mask=mask.reshape(H, W), tri=tri.reshape(H, W),
                    bary=bary.reshape(H, W, 2), normal=torch.zeros(H, W, 3, dtype=torch.float32, device=dev), color=col)
    idx = triangles.to(torch.int64).reshape(-1, 3)[tri.clamp(min=0).to(torch.int64)]  # [N,3]; row 0 stands in off the mesh
    w = torch.stack([1.0 - bary[:, 0] - bary[:, 1], bary[:, 0], bary[:, 1]], dim=1)  # [N,3]
    zero = torch.zeros(o.shape[0], 3, dtype=torch.float32, device=dev)

    def mix(attr):
        return (w[:, :, None] * attr.to(torch.float32).reshape(-1, 3)[idx]).sum(dim=1)

    def unit(n):
        length = torch.linalg.norm(n, dim=1, keepdim=True)
        ok = torch.isfinite(length) & (length > 0)
        return torch.where(ok, n / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(n))
    if normals is not None:
        nrm = unit(mix(normals))
    else:
        c = vertices.to(torch.float32).reshape(-1, 3)[idx]  # [N,3,3]
        face = torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        nrm = unit(torch.where(((face * d).sum(dim=1, keepdim=True) > 0), -face, face))
    nrm = torch.where(mask[:, None], nrm, zero)
    col = None
    if colors is not None:
        bg = torch.as_tensor(bg_color, dtype=torch.float32, device=dev).expand(3)
        col = torch.where(mask[:, None], mix(colors), bg[None, :]).reshape(H, W, 3)
    if texture is not None:
        if texture_cell is None:
            raise ValueError("texture needs texture_cell, the cell edge S it was baked with")
        if texture.dim() == 4:
            col = sample_sh_texture(texture, texture_cell, int(triangles.shape[0]), tri, bary, d, bg_color=bg_color).reshape(H, W, 3)
        else:
            col = sample_texture(texture, texture_cell, int(triangles.shape[0]), tri, bary, bg_color=bg_color).reshape(H, W, 3)
    return dict(depth=torch.where(mask, t, torch.zeros_like(t)).reshape(H, W), mask=mask.reshape(H, W), tri=tri.reshape(H, W),
                bary=bary.reshape(H, W, 2), normal=nrm.reshape(H, W, 3), color=col)


@torch.no_grad()
def evaluate_mesh_views(vertices, triangles, colors, poses, intrinsics, H, W, truth, bg_color=1.0, grid=None, keep_images=False,
                        texture=None, texture_cell=None):
    """Render the coloured mesh from poses [P,4,4] (render_mesh) and measure each view's colour image against `truth` the way
    pvd.metrics.evaluate_views does for a model: a tensor [P,H,W,3], or a callable (rays_o, rays_d) -> [H*W,3].  Returns
    ImageMeter.report() plus "coverage", the share of all pixels that hit the mesh (and, with keep_images, the views under
    "images").  texture, texture_cell: render_mesh's -- the views are coloured from the atlas (a flat one, or a 4-D SH atlas seen along
    each view's rays), and colors may be None."""
    from .metrics import ImageMeter
    from .scene import get_rays
    meter = ImageMeter()
    images, hit, pixels = [], None, 0
    for v, pose in enumerate(poses):
        pose = torch.as_tensor(pose, dtype=torch.float32, device=vertices.device).reshape(4, 4)
        if texture is None:
            out = render_mesh(vertices, triangles, pose, intrinsics, H, W, colors=colors, bg_color=bg_color, grid=grid)
        else:
            out = render_mesh(vertices, triangles, pose, intrinsics, H, W, colors=colors, bg_color=bg_color, grid=grid, texture=texture,
                              texture_cell=texture_cell)
        if callable(truth):
            r = get_rays(pose[None], intrinsics, int(H), int(W), -1)
            gt = truth(r["rays_o"], r["rays_d"])
        else:
            gt = truth[v]
        meter.update(out["color"], gt.to(vertices.device).float().reshape(H, W, 3))
        n = out["mask"].sum()
        hit = n if hit is None else hit + n
        pixels += int(H) * int(W)
        if keep_images:
            images.append(out["color"])
    report = meter.report()
    report["coverage"] = float(hit) / pixels if pixels else float("nan")
    if keep_images:
        report["images"] = images
    return report


# ------------------------------------------------------------------------------------------------ inside and outside: winding numbers
def mesh_winding(points, vertices, triangles, bmin=None, bmax=None, grid=None):
    """w [N] int32 on the device: the winding number of every row of points [N,3] about the mesh (vertices [V,3] f32, triangles [T,3]
    int32) -- the signed crossings of the ray along +z, in unfused float64 with a tie rule that counts a ray through a shared edge or
    vertex once (include/pvd_hip_mesh_winding.h; csrc/mesh_winding.hip).  +1 inside a closed mesh with outward normals (extract_mesh's
    orientation), 0 outside; pvd_hip.MESH_WINDING_INVALID for a row that is not finite.  Triangles with an index outside [0, V) or a
    corner that is not finite are ignored.  The grid of grid^2 cells (default: default_grid(T); 1 .. 1024, anything else raises) lies
    over the x / y extent of bmin .. bmax (default: the bounding box of the finite vertices); neither changes a bit of the result."""
    import pvd_hip
    points = points.to(torch.float32).reshape(-1, 3).contiguous()
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    T, G, pairs, ws = _tri_grid("mesh_winding", vertices, triangles, bmin, bmax, grid)
    w = torch.empty(points.shape[0], dtype=torch.int32, device=vertices.device)
    pvd_hip.mesh_winding_points(points, T, G, pairs, ws, w)
    return w


def mesh_contains(points, vertices, triangles, bmin=None, bmax=None, grid=None):
    """bool [N] on the device: mesh_winding(...) != 0; False for a row that is not finite."""
    import pvd_hip
    w = mesh_winding(points, vertices, triangles, bmin, bmax, grid)
    return (w != 0) & (w != pvd_hip.MESH_WINDING_INVALID)


def voxelize_mesh(vertices, triangles, R, bmin, bmax, grid=None, return_totals=False):
    """w [R,R,R] int32 on the device, x-major as density_field fills its volume: the winding number of the mesh at every point of the
    R^3 lattice of the box bmin .. bmax (R: 2 .. 1024), bit for bit what mesh_winding returns for those points, a column of R points
    per ray.  (w != 0).float() is a field that extract_mesh(., 0.5, bmin, bmax), label_components and drop_components accept.
    return_totals=True: (w, dict) with `inside` (points with w != 0), `positive` (w > 0), `leaky_columns` (columns of the lattice
    whose crossings do not sum to 0: not 0 for a mesh that is open, or inconsistently oriented, above that column) and `max_abs`."""
    import pvd_hip
    dev = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    R = int(R)
    lo, hi = _box(bmin, bmax, dev)
    T, G, pairs, ws = _tri_grid("mesh_winding", vertices, triangles, None, None, grid)
    w = torch.empty(R, R, R, dtype=torch.int32, device=dev) if 2 <= R <= pvd_hip.MESH_WINDING_MAX_R else torch.empty(0, dtype=torch.int32, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    pvd_hip.mesh_winding_lattice(R, lo, hi, T, G, pairs, ws, w, totals)
    if not return_totals:
        return w
    return w, dict(zip(pvd_hip.MESH_WINDING_TOTALS, (int(x) for x in totals.tolist())))


def mesh_signed_distance(points, vertices, triangles, max_dist, bmin=None, bmax=None, grid=None):
    """(sdf [N] f32, tri [N] int32), device tensors: mesh_distance's distance and triangle, the distance with a sign -- positive inside
    the mesh (mesh_contains), negative outside: the project's convention that inside is the larger value.  The magnitude and tri are
    mesh_distance's bits: a row saturated at max_dist stays at max_dist, with its sign, and a row that is not finite stays NaN."""
    dist, tri = mesh_distance(points, vertices, triangles, max_dist, bmin, bmax, grid)
    inside = mesh_contains(points, vertices, triangles, bmin, bmax, grid)
    return torch.where(inside, dist, -dist), tri


@torch.no_grad()
def mesh_to_sdf(vertices, triangles, R, bmin, bmax, max_dist, chunk=1 << 21):
    """sdf [R,R,R] f32 on the device: the signed distance (positive inside, saturated at +-max_dist) from every point of the R^3
    lattice of the box bmin .. bmax to the mesh -- the sign from voxelize_mesh, the magnitude from the point-to-mesh distance at
    lattice points made on the device `chunk` at a time (the float32 lattice of include/pvd_hip_mesh_winding.h).
    extract_mesh(mesh_to_sdf(...), 0.0, bmin, bmax) is a remesh at another resolution."""
    import pvd_hip
    dev = vertices.device
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    R = int(R)
    w = voxelize_mesh(vertices, triangles, R, bmin, bmax)
    lo, hi = _box(bmin, bmax, dev)
    # a tensor divisor: a true float32 division (a Python scalar divisor is turned into a multiplication by its rounded reciprocal)
    steps = torch.arange(R, dtype=torch.float32, device=dev)[:, None] / torch.full((1, 1), float(R - 1), dtype=torch.float32, device=dev)
    axes = steps * (hi - lo)[None, :] + lo[None, :]  # [R,3]
    T = int(triangles.shape[0])
    G = default_grid(T)
    box_lo, box_hi = _finite_box(vertices)
    ws = torch.empty(pvd_hip.mesh_dist_workspace_bytes(T, G), dtype=torch.uint8, device=dev)
    pvd_hip.mesh_dist_build(vertices, triangles, box_lo, box_hi, G, ws)
    sdf = torch.empty(R, R, R, dtype=torch.float32, device=dev)
    flat, N = sdf.view(-1), R ** 3
    for s in range(0, N, int(chunk)):
        n = torch.arange(s, min(s + int(chunk), N), dtype=torch.int64, device=dev)
        pts = torch.stack([axes[n // (R * R), 0], axes[(n // R) % R, 1], axes[n % R, 2]], dim=1).contiguous()
        tri = torch.empty(n.numel(), dtype=torch.int32, device=dev)
        pvd_hip.mesh_dist_query(pts, T, G, ws, float(max_dist), flat[s:s + n.numel()], tri)
    inside = (w != 0) & (w != pvd_hip.MESH_WINDING_INVALID)
    return torch.where(inside, sdf, -sdf)


def _volume_overlap(va, ta, vb, tb, R):
    """compare_meshes(volume=R): both meshes voxelised on one R^3 lattice over the joint bounding box of their finite vertices."""
    R = int(R)
    lo_a, hi_a = _finite_box(va)
    lo_b, hi_b = _finite_box(vb)
    lo, hi = torch.minimum(lo_a, lo_b), torch.maximum(hi_a, hi_b)
    wa, tot_a = voxelize_mesh(va, ta, R, lo, hi, return_totals=True)
    wb, tot_b = voxelize_mesh(vb, tb, R, lo, hi, return_totals=True)
    in_a, in_b = wa != 0, wb != 0
    both, either = (int(x) for x in torch.stack([(in_a & in_b).sum(), (in_a | in_b).sum()]).tolist())
    cell = 1.0
    for l, h in zip(lo.tolist(), hi.tolist()):
        cell *= (h - l) / (R - 1)  # the lattice spacing of the axis
    return dict(iou=both / either if either else 0.0, volume_a=tot_a["inside"] * cell, volume_b=tot_b["inside"] * cell,
                leaky_a=tot_a["leaky_columns"], leaky_b=tot_b["leaky_columns"])


# ------------------------------------------------------------------------------------------------ texture atlases
def _is_atlas(S):
    """True for adaptive_atlas's dict where the texture functions take the cell edge S."""
    return isinstance(S, dict) and "slot" in S and "order" in S and "counts" in S


def _atlas_for(S, T):
    if int(S["triangles"]) != int(T):
        raise ValueError("the adaptive atlas was built for %d triangles, the mesh has %d" % (int(S["triangles"]), int(T)))
    return S


def adaptive_atlas(vertices, triangles, density, max_cell=64):
    """The area-adaptive atlas of csrc/pvd_hip_mesh_atex.h for the mesh: every triangle gets the smallest cell edge of 4, 8, 16, 32, 64
    texels (at most max_cell) that gives it `density` texels per unit length along its longest edge, and the triangles of one cell size
    are packed into one band of the image in the order of their index (csrc/mesh_atex.hip: a counting sort by scans, no atomics, the
    same bits every run).  A dict: slot [T] int32 (class << 28 | rank) and order [T] int32 on the device, counts (five integers),
    capped (triangles that needed more than max_cell), density, triangles = T and layout = dict(width, height, y0, rows, cells_per_row,
    cell: five numbers each, triangles).  texture_layout, texture_uv, texture_points, bake_texture, sample_texture and
    render_mesh(texture_cell=...) take it in place of the integer S."""
    import pvd_hip
    if int(max_cell) not in pvd_hip.MESH_ATEX_CELLS:
        raise ValueError("max_cell must be one of %s, got %r" % (pvd_hip.MESH_ATEX_CELLS, max_cell))
    if not float(density) > 0.0 or float(density) == float("inf"):
        raise ValueError("density must be positive and finite, got %r" % (density,))
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    dev, T = vertices.device, int(triangles.shape[0])
    slot = torch.empty(T, dtype=torch.int32, device=dev)
    order = torch.empty(T, dtype=torch.int32, device=dev)
    totals = torch.zeros(6, dtype=torch.int32, device=dev)
    ws = torch.empty(pvd_hip.mesh_atex_workspace_bytes(T), dtype=torch.uint8, device=dev)
    pvd_hip.mesh_atex_build(vertices, triangles, float(density), pvd_hip.MESH_ATEX_CELLS.index(int(max_cell)), ws, slot, order, totals)
    totals = [int(v) for v in totals.tolist()]
    counts = tuple(totals[:5])
    Wt, Ht, y0, rows, C = pvd_hip.mesh_atex_layout(counts)
    return dict(slot=slot, order=order, counts=counts, capped=totals[5], density=float(density), triangles=T,
                layout=dict(width=Wt, height=Ht, y0=y0, rows=rows, cells_per_row=C, cell=tuple(pvd_hip.MESH_ATEX_CELLS), triangles=T))


def texture_layout(T, S):
    """dict(cells_per_row, rows, width, height, cell, triangles) of the per-triangle atlas of include/pvd_hip_mesh_tex.h: two triangles
    share a square cell of S x S texels (S 4 .. 64), C cells per row with C the smallest integer whose square holds ceil(T / 2) cells.
    A side above 16384 texels raises.  S = adaptive_atlas's dict: its layout (width, height, and per class y0, rows, cells_per_row, cell)."""
    import pvd_hip
    if _is_atlas(S):
        return dict(_atlas_for(S, T)["layout"])
    C, rows, Wt, Ht = pvd_hip.mesh_tex_layout(int(T), int(S))
    return dict(cells_per_row=C, rows=rows, width=Wt, height=Ht, cell=int(S), triangles=int(T))


def texture_uv(T, S, device=None):
    """[T,3,2] f32: the texture coordinates of the three corners of every triangle in the OBJ convention (u to the right, v up, the
    image's first row at v = 1): the centres of the texels that hold the corners' baked values.  The header's closed form, in torch
    (with an adaptive atlas: per triangle from its slot, csrc/pvd_hip_mesh_atex.h)."""
    lay = texture_layout(T, S)
    if _is_atlas(S):
        slot = S["slot"].to(torch.int64) if device is None else S["slot"].to(device=device, dtype=torch.int64)
        c, k = slot >> 28, (slot & 0x0fffffff) // 2
        odd = (slot & 1) == 1
        cell = torch.tensor(lay["cell"], dtype=torch.int64, device=slot.device)[c]
        C = torch.tensor(lay["cells_per_row"], dtype=torch.int64, device=slot.device)[c]
        y0 = torch.tensor(lay["y0"], dtype=torch.int64, device=slot.device)[c]
        ax = (k % C) * cell + torch.where(odd, cell - 1, torch.zeros_like(cell))
        ay = y0 + (k // C) * cell + torch.where(odd, cell - 1, torch.zeros_like(cell))
        step = torch.where(odd, 3 - cell, cell - 3)
        X = torch.stack([ax, ax + step, ax], dim=1).to(torch.float64) + 0.5
        Y = torch.stack([ay, ay, ay + step], dim=1).to(torch.float64) + 0.5
        return torch.stack([X / lay["width"], 1.0 - Y / lay["height"]], dim=2).to(torch.float32)
    C, Wt, Ht, S, m = lay["cells_per_row"], lay["width"], lay["height"], int(S), int(S) - 3
    f = torch.arange(int(T), dtype=torch.int64, device=device)
    k, odd = f // 2, (f % 2) == 1
    ax = (k % C) * S + torch.where(odd, S - 1, 0)
    ay = (k // C) * S + torch.where(odd, S - 1, 0)
    step = torch.where(odd, -m, m)
    X = torch.stack([ax, ax + step, ax], dim=1).to(torch.float64) + 0.5
    Y = torch.stack([ay, ay, ay + step], dim=1).to(torch.float64) + 0.5
    return torch.stack([X / Wt, 1.0 - Y / Ht], dim=2).to(torch.float32)


def texture_points(vertices, triangles, S, normals=None, rows=None):
    """(x, n) [(row1 - row0) * width, 3] f32 on the device: the surface point and the normal of every texel of the image rows
    rows = (row0, row1) (default: the whole atlas) of the mesh's atlas (csrc/mesh_tex.hip).  n: the weights of x on the vertex normals
    [V,3], left unnormalised, or the face normal without them.  Six NaNs for a texel nothing owns and for the texels of a triangle with an
    index outside [0, V) or a corner (or given normal) that is not finite.  S = adaptive_atlas's dict: the same on that atlas
    (csrc/mesh_atex.hip)."""
    import pvd_hip
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    triangles = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    if normals is not None:
        normals = normals.to(torch.float32).reshape(-1, 3).contiguous()
    lay = texture_layout(int(triangles.shape[0]), S)
    row0, row1 = (0, lay["height"]) if rows is None else (int(rows[0]), int(rows[1]))
    count = max(row1 - row0, 0) * lay["width"]
    x = torch.empty(count, 3, dtype=torch.float32, device=vertices.device)
    n = torch.empty(count, 3, dtype=torch.float32, device=vertices.device)
    if _is_atlas(S):
        pvd_hip.mesh_atex_points(vertices, triangles, normals, S["counts"], S["order"], row0, row1, x, n)
    else:
        pvd_hip.mesh_tex_points(vertices, triangles, normals, int(S), row0, row1, x, n)
    return x, n


def _unit_rows(n):
    length = torch.linalg.norm(n, dim=1, keepdim=True)
    ok = torch.isfinite(length) & (length > 0)
    return torch.where(ok, n / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(n))


@torch.no_grad()
def bake_texture(source, vertices, triangles, S, normals=None, chunk=1 << 20):
    """dict(texture [Ht,Wt,3] f32 in [0,1], uv [T,3,2] f32, layout): the colour of `source` at the surface point of every texel of the
    mesh's atlas (texture_layout, texture_points).  source: a model -- vertex_colors(model, x, n / |n|), the colour head seen straight
    on, as the vertex colours are taken -- or a callable (x [M,3], n_unit [M,3]) -> [M,3].  Baked in bands of whole image rows of about
    `chunk` texels; texels nothing owns, and those of invalid triangles, get the colour 0 and never reach the source.
    S = adaptive_atlas's dict: the bake on that atlas; the dict then also holds texture_cell = the atlas, which is what sample_texture,
    render_mesh and evaluate_mesh_views take in place of S."""
    T = int(triangles.reshape(-1, 3).shape[0])
    lay = texture_layout(T, S)
    Wt, Ht = lay["width"], lay["height"]
    texture = torch.empty(Ht, Wt, 3, dtype=torch.float32, device=vertices.device)
    band = max(1, int(chunk) // Wt)
    is_model = hasattr(source, "aabb_infer")
    for row0 in range(0, Ht, band):
        row1 = min(row0 + band, Ht)
        x, n = texture_points(vertices, triangles, S, normals=normals, rows=(row0, row1))
        if is_model:  # rows that are not finite come back as colour 0
            rgb = vertex_colors(source, x, _unit_rows(n), chunk=chunk)
        else:
            good = torch.isfinite(x).all(dim=1) & torch.isfinite(n).all(dim=1)
            rgb = torch.zeros_like(x)
            if bool(good.any()):
                rgb[good] = source(x[good].contiguous(), _unit_rows(n[good]).contiguous()).to(torch.float32).reshape(-1, 3).clamp(0.0, 1.0)
        texture[row0:row1] = rgb.reshape(row1 - row0, Wt, 3)
    out = dict(texture=texture, uv=texture_uv(T, S, device=vertices.device), layout=lay)
    if _is_atlas(S):
        out["texture_cell"] = S
    return out


def sample_texture(texture, S, T, tri, bary, bg_color=1.0):
    """[..., 3] f32 on the device: the bilinear lookup of texture [Ht,Wt,3] (the atlas of T triangles at the cell edge S) at the hits
    (tri [...] int32, bary [..., 2] f32) of mesh_raycast; bg_color (a float or 3 floats) where tri is -1.  Reads the hit triangle's own
    cell only (include/pvd_hip_mesh_tex.h; csrc/mesh_tex.hip).  S = adaptive_atlas's dict: the lookup on that atlas
    (csrc/mesh_atex.hip)."""
    import pvd_hip
    dev = texture.device
    texture = texture.to(torch.float32).contiguous()
    shape = tuple(tri.shape)
    tri = tri.to(torch.int32).reshape(-1).contiguous()
    bary = bary.to(torch.float32).reshape(-1, 2).contiguous()
    bg = torch.as_tensor(bg_color, dtype=torch.float32, device=dev).expand(3).contiguous()
    color = torch.empty(int(tri.shape[0]), 3, dtype=torch.float32, device=dev)
    if _is_atlas(S):
        pvd_hip.mesh_atex_sample(texture, int(T), _atlas_for(S, T)["counts"], S["slot"], tri, bary, bg, color)
    else:
        pvd_hip.mesh_tex_sample(texture, int(T), int(S), tri, bary, bg, color)
    return color.reshape(shape + (3,))


def _png_chunk(kind, data):
    import struct
    import zlib
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, image):
    """8-bit RGB PNG of image [H,W,3] (floats in [0,1]: round(clamp(c, 0, 1) * 255), NaN as 0; or uint8), first row on top: stdlib zlib,
    filter 0 on every row, one IDAT chunk."""
    import struct
    import zlib

    import numpy as np
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("image must be [H,W,3] with H, W >= 1")
    if a.dtype != np.uint8:
        with np.errstate(invalid="ignore"):
            a = np.rint(np.clip(np.nan_to_num(a.astype(np.float32), nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)  # the filter byte 0, then the row
    rows[:, 1:] = a.reshape(H, 3 * W)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)))
        f.write(_png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(_png_chunk(b"IEND", b""))
    return path


def read_png(path):
    """[H,W,3] f32 in [0,1] (byte / 255), a host tensor, of a file write_png wrote: 8-bit RGB, not interlaced, filter 0 on every row (any
    number of IDAT chunks); anything else raises."""
    import struct
    import zlib

    import numpy as np
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s: not a PNG" % path)
    pos, head, body = 8, None, b""
    while pos + 12 <= len(data):
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        chunk = data[pos + 8:pos + 8 + n]
        if len(chunk) != n or struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + chunk) & 0xffffffff):
            raise ValueError("%s: a damaged chunk" % path)
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", chunk)
        elif kind == b"IDAT":
            body += chunk
        elif kind == b"IEND":
            break
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError("%s: not an 8-bit RGB PNG without interlace" % path)
    W, H = head[:2]
    rows = np.frombuffer(zlib.decompress(body), np.uint8)
    if rows.size != H * (1 + 3 * W):
        raise ValueError("%s: truncated" % path)
    rows = rows.reshape(H, 1 + 3 * W)
    if np.any(rows[:, 0] != 0):
        raise ValueError("%s: a row filter other than 0" % path)
    return torch.from_numpy(rows[:, 1:].reshape(H, W, 3).astype(np.float32) / np.float32(255.0))


def write_obj(path, vertices, triangles, uv, texture_file, normals=None):
    """Wavefront OBJ with a texture: `v` per vertex, `vn` per vertex where normals [V,3] are given, three `vt` per triangle (uv [T,3,2],
    texture_uv's), `f a/t` or `f a/t/n` (1-based), and next to it an .mtl of the same name with one material whose map_Kd is
    texture_file (a name relative to the OBJ).  Floats are written with 9 significant digits: float32 comes back bit for bit."""
    import os

    import numpy as np

    def host(a, dtype, cols):
        return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dtype).reshape(-1, cols)
    v, t, w = host(vertices, np.float32, 3), host(triangles, np.int64, 3), host(uv, np.float32, 2)
    if len(w) != 3 * len(t):
        raise ValueError("uv must be [T,3,2]")
    mtl = os.path.splitext(path)[0] + ".mtl"
    lines = ["mtllib %s" % os.path.basename(mtl), "usemtl material0"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    if normals is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in host(normals, np.float32, 3).tolist()]
    lines += ["vt %.9g %.9g" % tuple(r) for r in w.tolist()]
    for f, (a, b, c) in enumerate(t.tolist()):
        k = 3 * f + 1
        if normals is not None:
            lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d" % (a + 1, k, a + 1, b + 1, k + 1, b + 1, c + 1, k + 2, c + 1))
        else:
            lines.append("f %d/%d %d/%d %d/%d" % (a + 1, k, b + 1, k + 1, c + 1, k + 2))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(mtl, "w") as f:
        f.write("newmtl material0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s\n" % texture_file)
    return path


def read_obj(path):
    """dict(vertices [V,3] f32, triangles [T,3] int32, uv [T,3,2] f32, normals [V,3] f32 | None, mtllib, texture_file) of a file
    write_obj wrote, as host tensors: `v`, `vn`, `vt`, triangular `f a/t` or `f a/t/n` with the normal's index equal to the vertex's,
    `mtllib`, `usemtl`; texture_file is the map_Kd of the .mtl next to the file (None where there is none).  Anything else raises."""
    import os

    import numpy as np
    v, vn, vt, fv, ft, mtllib = [], [], [], [], [], None
    with open(path) as f:
        for line in f:
            words = line.split()
            if not words or words[0].startswith("#") or words[0] == "usemtl":
                continue
            if words[0] == "v" and len(words) == 4:
                v.append([float(x) for x in words[1:]])
            elif words[0] == "vn" and len(words) == 4:
                vn.append([float(x) for x in words[1:]])
            elif words[0] == "vt" and len(words) == 3:
                vt.append([float(x) for x in words[1:]])
            elif words[0] == "f" and len(words) == 4:
                parts = [w.split("/") for w in words[1:]]
                if any(len(p) not in (2, 3) or (len(p) == 3 and p[2] != p[0]) for p in parts):
                    raise ValueError("%s: unexpected face %r" % (path, line))
                fv.append([int(p[0]) - 1 for p in parts])
                ft.append([int(p[1]) - 1 for p in parts])
            elif words[0] == "mtllib" and len(words) == 2:
                mtllib = words[1]
            else:
                raise ValueError("%s: unexpected line %r" % (path, line))
    texture_file = None
    if mtllib is not None and os.path.exists(os.path.join(os.path.dirname(path), mtllib)):
        with open(os.path.join(os.path.dirname(path), mtllib)) as f:
            for line in f:
                if line.startswith("map_Kd "):
                    texture_file = line[len("map_Kd "):].strip()
    vt = np.array(vt, np.float32).reshape(-1, 2)
    ft = np.array(ft, np.int64).reshape(-1, 3)
    return dict(vertices=torch.from_numpy(np.array(v, np.float32).reshape(-1, 3)),
                triangles=torch.from_numpy(np.array(fv, np.int32).reshape(-1, 3)), uv=torch.from_numpy(vt[ft].reshape(-1, 3, 2)),
                normals=torch.from_numpy(np.array(vn, np.float32).reshape(-1, 3)) if vn else None, mtllib=mtllib,
                texture_file=texture_file)


# ------------------------------------------------------------------------------------------------ view-dependent texture atlases
_SH_Y0 = 0.282094806  # Y_0 of csrc/pvd_hip_mesh_shtex.h


def _sh_bands(degree):
    L = int(degree)
    if not 1 <= L <= 4:
        raise ValueError("degree (the number of SH bands) must be 1 .. 4, got %r" % (degree,))
    return L


def _sh_basis_host(d, L):
    """The header's sixteen polynomials on a host tensor: the same float32 operations in the same order, each a torch operation of its
    own (eager torch fuses nothing)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]

    def c(v):
        return torch.tensor(v, dtype=torch.float32)
    Y = [c(0.282094806).expand(d.shape[0])]
    if L > 1:
        Y += [c(-0.488602519) * y, c(0.488602519) * z, c(-0.488602519) * x]
    if L > 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        Y += [c(1.09254849) * xy, c(-1.09254849) * yz, c(0.946174681) * zz - c(0.31539157), c(-1.09254849) * xz,
              c(0.546274245) * (xx - yy)]
    if L > 3:
        Y += [c(-0.590043604) * (y * (c(3.0) * xx - yy)), c(2.89061141) * (xy * z), (c(0.457045794) - c(2.28522897) * zz) * y,
              (c(1.86588168) * zz - c(1.11952901)) * z, (c(0.457045794) - c(2.28522897) * zz) * x, c(1.44530571) * (z * (xx - yy)),
              c(-0.590043604) * (x * (xx - c(3.0) * yy))]
    return torch.stack(Y, dim=1)


def sh_basis(dirs, degree):
    """[N, K] f32, K = degree^2: the real spherical harmonics of csrc/pvd_hip_mesh_shtex.h (index l * l + l + m, the signs of the
    direction encoder's basis) at dirs [N,3], used as given and not normalised.  A device tensor goes through the kernel
    (csrc/mesh_shtex.hip); a host tensor -- the few dozen fitting directions of sh_fit_matrix -- is evaluated on the host by the same
    float32 operations in the same order, so both give the same bits."""
    L = _sh_bands(degree)
    dirs = dirs.to(torch.float32).reshape(-1, 3).contiguous()
    if not dirs.is_cuda:
        return _sh_basis_host(dirs, L)
    import pvd_hip
    out = torch.empty(int(dirs.shape[0]), L * L, dtype=torch.float32, device=dirs.device)
    pvd_hip.mesh_shtex_basis(dirs, L, out)
    return out


def sh_fit_matrix(dirs, degree):
    """P [K, D] f32 on dirs' device: the least-squares fit of K = degree^2 SH coefficients to values at the D directions dirs [D,3] --
    the pseudo-inverse of Y = sh_basis(dirs, degree) [D,K], taken in float64 on the host and rounded once.  ValueError where D < K, and
    where Y's smallest singular value is below 1e-3 of its largest: a degenerate set (directions in a plane, say) would otherwise bake
    coefficients that mean nothing."""
    import numpy as np
    L = _sh_bands(degree)
    K = L * L
    D = int(dirs.reshape(-1, 3).shape[0])
    if D < K:
        raise ValueError("%d directions cannot fit %d coefficients" % (D, K))
    Y = sh_basis(dirs, L).to(torch.float64).cpu().numpy()
    sv = np.linalg.svd(Y, compute_uv=False)
    if not np.all(np.isfinite(sv)) or sv[-1] < 1e-3 * sv[0]:
        raise ValueError("the directions do not determine %d SH coefficients: singular values %.3g .. %.3g" % (K, sv[-1], sv[0]))
    return torch.from_numpy(np.linalg.pinv(Y).astype(np.float32)).to(dirs.device)


def _colors_along(model, x, d, chunk, autocast=True):
    """[M,3] f32 in [0,1]: rgb = model(x, d)[1], the colour head seen along the direction of travel d, as vertex_colors asks it with
    d = -normal.  Rows that are not finite never reach the model and get the colour 0."""
    M = int(x.shape[0])
    out = torch.empty(M, 3, dtype=torch.float32, device=x.device)
    aabb = model.aabb_infer.to(device=x.device, dtype=torch.float32)
    centre = (aabb[:3] + aabb[3:]) * 0.5
    down = torch.tensor([0.0, 0.0, -1.0], device=x.device)
    for s in range(0, M, int(chunk)):
        xs, ds = x[s:s + int(chunk)], d[s:s + int(chunk)]
        bad = ~(torch.isfinite(xs).all(dim=1) & torch.isfinite(ds).all(dim=1))
        xs = torch.where(bad[:, None], centre[None, :], xs).contiguous()
        ds = torch.where(bad[:, None], down[None, :], ds).contiguous()
        with torch.autocast("cuda", dtype=torch.float16, enabled=bool(autocast)):
            rgb = model(xs, ds)[1]
        out[s:s + xs.shape[0]] = torch.where(bad[:, None], torch.zeros_like(xs), rgb.to(torch.float32).clamp(0.0, 1.0))
    return out


def _no_sh_atlas(S):
    if _is_atlas(S):
        raise ValueError("SH atlases take an integer cell edge: the adaptive atlas (adaptive_atlas) is for flat textures only")


@torch.no_grad()
def bake_sh_texture(source, vertices, triangles, S, degree=3, dirs=None, normals=None, chunk=1 << 20, batch=8):
    """dict(texture [Ht,Wt,K,3] f32, uv [T,3,2] f32, layout, degree, diffuse [Ht,Wt,3] f32): per texel of the mesh's atlas
    (texture_layout, texture_points) the K = degree^2 SH coefficients per channel of the colour of `source` as a function of the
    direction of travel d of a ray that sees the texel's surface point (csrc/pvd_hip_mesh_shtex.h).  dirs [D,3]: the fitting
    directions, one full-sphere set for every texel (default exposure_directions(64)); a direction that would look at a texel from
    behind is mirrored in its tangent plane, so no colour is taken from behind the surface.  source: a model -- rgb = model(x, d)[1],
    the colour head as vertex_colors asks it -- or a callable (x [M,3], d [M,3]) -> [M,3].  The bake costs D colour queries per texel:
    in bands of whole image rows of about `chunk` texels and `batch` directions at a time, projected onto the basis as they come
    (sh_fit_matrix).  Texels nothing owns, and those of invalid triangles, get all-zero coefficients and never reach the source.
    diffuse = clamp(coef[..., 0, :] * Y_0, 0, 1), the view-independent part: what an OBJ / PNG can carry.  sample_sh_texture and
    render_mesh(texture=...) evaluate the atlas at a ray's direction."""
    import pvd_hip
    _no_sh_atlas(S)
    L = _sh_bands(degree)
    K = L * L
    dev = vertices.device
    T = int(triangles.reshape(-1, 3).shape[0])
    lay = texture_layout(T, S)
    Wt, Ht = lay["width"], lay["height"]
    U = (exposure_directions(64) if dirs is None else dirs).to(torch.float32).reshape(-1, 3)
    P = sh_fit_matrix(U, L).to(dev)
    U = U.to(dev).contiguous()
    D, batch = int(U.shape[0]), max(1, int(batch))
    texture = torch.empty(Ht, Wt, K, 3, dtype=torch.float32, device=dev)
    band = max(1, int(chunk) // Wt)
    is_model = hasattr(source, "aabb_infer")
    for row0 in range(0, Ht, band):
        row1 = min(row0 + band, Ht)
        x, n = texture_points(vertices, triangles, S, normals=normals, rows=(row0, row1))
        good = torch.isfinite(x).all(dim=1) & torch.isfinite(n).all(dim=1)
        rows = torch.zeros(int(x.shape[0]), K, 3, dtype=torch.float32, device=dev)
        xg, ng = x[good].contiguous(), n[good].contiguous()
        M = int(xg.shape[0])
        if M:
            coef = torch.empty(M, K, 3, dtype=torch.float32, device=dev)
            for j0 in range(0, D, batch):
                Uj = U[j0:j0 + batch].contiguous()
                J = int(Uj.shape[0])
                d = torch.empty(J, M, 3, dtype=torch.float32, device=dev)
                pvd_hip.mesh_shtex_dirs(ng, Uj, d)
                xq = xg[None].expand(J, M, 3).reshape(-1, 3)
                if is_model:
                    rgb = _colors_along(source, xq, d.reshape(-1, 3), chunk)
                else:
                    rgb = source(xq.contiguous(), d.reshape(-1, 3)).to(torch.float32)
                pvd_hip.mesh_shtex_project(rgb.reshape(J, M, 3).contiguous(), P[:, j0:j0 + J].contiguous(), L, coef, j0 == 0)
            rows[good] = coef
        texture[row0:row1] = rows.reshape(row1 - row0, Wt, K, 3)
    diffuse = (texture[:, :, 0, :] * torch.tensor(_SH_Y0, dtype=torch.float32, device=dev)).clamp(0.0, 1.0)
    return dict(texture=texture, uv=texture_uv(T, S, device=dev), layout=lay, degree=L, diffuse=diffuse)


def sample_sh_texture(texture, S, T, tri, bary, dirs, bg_color=1.0):
    """[..., 3] f32 in [0,1] on the device: the SH atlas texture [Ht,Wt,K,3] (bake_sh_texture's, T triangles at the cell edge S)
    evaluated at the directions dirs [..., 3] of the rays and looked up bilinearly at their hits (tri [...] int32, bary [..., 2] f32,
    mesh_raycast's); bg_color (a float or 3 floats) where tri is -1.  K = 1, 4, 9 or 16 gives the number of bands.  Reads the hit
    triangle's own cell only (csrc/pvd_hip_mesh_shtex.h; csrc/mesh_shtex.hip)."""
    import math

    import pvd_hip
    _no_sh_atlas(S)
    if texture.dim() != 4:
        raise ValueError("an SH atlas is [Ht,Wt,K,3]")
    K = int(texture.shape[2])
    L = math.isqrt(K)
    if L * L != K:
        raise ValueError("K = %d coefficients per channel is not a square" % K)
    L = _sh_bands(L)
    dev = texture.device
    texture = texture.to(torch.float32).contiguous()
    shape = tuple(tri.shape)
    tri = tri.to(torch.int32).reshape(-1).contiguous()
    bary = bary.to(torch.float32).reshape(-1, 2).contiguous()
    dirs = dirs.to(torch.float32).reshape(-1, 3).contiguous()
    bg = torch.as_tensor(bg_color, dtype=torch.float32, device=dev).expand(3).contiguous()
    color = torch.empty(int(tri.shape[0]), 3, dtype=torch.float32, device=dev)
    pvd_hip.mesh_shtex_sample(texture, int(T), int(S), L, tri, bary, dirs, bg, color)
    return color.reshape(shape + (3,))


# ------------------------------------------------------------------------------------------- depth-map fusion (csrc/pvd_hip_mesh_tsdf.h)
class TSDFVolume:
    """The accumulators of a truncated signed distance volume over the R^3 lattice of the box bmin .. bmax (density_field's lattice):
    acc_d [R,R,R] (sum of w t), acc_w [R,R,R] (sum of w) and acc_c [R,R,R,3] (sum of w rgb; None without colour), f32 on the device,
    with the truncation distance tau and the number of views integrated so far.  Made by tsdf_volume."""

    def __init__(self, R, bmin, bmax, tau, acc_d, acc_w, acc_c):
        self.R, self.bmin, self.bmax, self.tau = R, bmin, bmax, tau
        self.acc_d, self.acc_w, self.acc_c = acc_d, acc_w, acc_c
        self.views = 0


def tsdf_volume(R, bmin, bmax, tau=None, with_color=True, device=None):
    """An empty TSDFVolume.  tau defaults to 3 lattice spacings of the longest box axis."""
    R = int(R)
    if R < 2:
        raise ValueError("R must be at least 2")
    if device is None:
        device = bmin.device if torch.is_tensor(bmin) else torch.device("cuda", torch.cuda.current_device())
    lo, hi = _box(bmin, bmax, device)
    if tau is None:
        tau = 3.0 * float((hi - lo).abs().max()) / (R - 1)
    tau = float(tau)
    if not 0.0 < tau < float("inf"):
        raise ValueError("tau must be positive and finite")
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=device)  # noqa: E731
    return TSDFVolume(R, lo, hi, tau, z(R, R, R), z(R, R, R), z(R, R, R, 3) if with_color else None)


def tsdf_integrate(acc, depth, poses, intrinsics, color=None, weight=None):
    """Adds the views to the volume `acc` (csrc/pvd_hip_mesh_tsdf.h, "Integrate"; one launch): depth [V,H,W] -- the distance along the
    unit ray of every pixel, +inf where the ray left the scene (free space), NaN or <= 0 where nothing is known --, poses [V,4,4]
    cam2world as get_rays takes them, intrinsics (fx, fy, cx, cy) for all views or [V,4], color [V,H,W,3] and weight [V,H,W] optional.
    A volume with colour takes views WITH colour only (ValueError otherwise: a view that added its weight but no colour would darken
    tsdf_vertex_colors, which divides the colour sums by the weight sums); a volume without colour ignores `color`.  Views may arrive in any number of calls: the result is, bit for
    bit, that of one call with all of them in the same order."""
    import pvd_hip
    dev = acc.acc_d.device
    f = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()  # noqa: E731
    depth, poses, color, weight = f(depth), f(poses), f(color), f(weight)
    V = int(depth.shape[0])
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev)
    if intrinsics.dim() == 1:
        intrinsics = intrinsics[None, :].expand(V, 4)
    if acc.acc_c is not None and color is None:
        raise ValueError("the volume accumulates colour: every call needs `color` (or make it with tsdf_volume(with_color=False))")
    with_color = acc.acc_c is not None
    pvd_hip.mesh_tsdf_integrate(depth, color if with_color else None, weight, poses, intrinsics.contiguous(), acc.R, acc.bmin, acc.bmax,
                                acc.tau, acc.acc_d, acc.acc_w, acc.acc_c if with_color else None)
    acc.views += V
    return acc


def tsdf_field(acc, min_weight=1.0, unknown=-1.0, return_totals=False):
    """field [R,R,R] f32 on the device, in [-1, 1] and POSITIVE OUTSIDE: acc_d / acc_w where acc_w >= min_weight, `unknown` elsewhere.
    unknown = -1 treats what no view observed as solid -- the interior behind the truncation band never is, so a watertight mesh needs
    it, and it also fills what no camera covers; unknown = +1 treats it as empty and leaves an inner shell where the band ends.
    extract_mesh meshes field > thresh as inside: hand it -field and the level 0 (extract_surface_tsdf does).  return_totals=True:
    (field, dict(observed, observed_inside, unknown)), one read-back."""
    import pvd_hip
    field = torch.empty(acc.R, acc.R, acc.R, dtype=torch.float32, device=acc.acc_d.device)
    totals = torch.empty(3, dtype=torch.int64, device=field.device)
    pvd_hip.mesh_tsdf_finalize(acc.acc_d, acc.acc_w, acc.R, float(min_weight), float(unknown), field, totals)
    if not return_totals:
        return field
    return field, dict(zip(pvd_hip.MESH_TSDF_TOTALS, (int(v) for v in totals.tolist())))


def tsdf_vertex_colors(acc, vertices, min_weight=1.0):
    """[V,3] f32 in [0,1] on the device: the fused colour at every vertex -- the trilinear blend of acc_c / acc_w over the observed ones
    of the 8 lattice points around it, renormalised; 0 for a vertex that is not finite, outside the box, or with no observed corner."""
    import pvd_hip
    if acc.acc_c is None:
        raise ValueError("the volume was made without colour")
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    colors = torch.empty_like(vertices)
    pvd_hip.mesh_tsdf_sample_color(acc.acc_c, acc.acc_w, acc.R, acc.bmin, acc.bmax, float(min_weight), vertices, colors)
    return colors


def tsdf_poses(n=64, radius=4.0, scale=0.8):
    """[n,4,4] f32 (a host tensor): the default cameras of extract_surface_tsdf -- pose_spherical views through nerf_matrix_to_ngp, as
    the synthetic scenes have them, looking at the origin from the points of exposure_directions' Fibonacci sphere: the elevation
    phi_i = -asin(z_i) covers both hemispheres, the azimuth theta_i is the sphere's."""
    import numpy as np

    from .scene import nerf_matrix_to_ngp, pose_spherical
    d = exposure_directions(int(n)).double().numpy()
    theta = np.degrees(np.arctan2(d[:, 1], d[:, 0]))
    phi = -np.degrees(np.arcsin(np.clip(d[:, 2], -1.0, 1.0)))
    return torch.from_numpy(np.stack([nerf_matrix_to_ngp(pose_spherical(float(t), float(p), float(radius)), scale)
                                      for t, p in zip(theta, phi)]).astype(np.float32))


@torch.no_grad()
def render_depth_maps(model, poses, intrinsics, H, W, min_opacity=0.5, free_opacity=0.05, max_steps=1024, ray_batch=1 << 16):
    """dict(depth [V,H,W], color [V,H,W,3], opacity [V,H,W]), f32 on the device: what tsdf_integrate wants, rendered by `model` on its
    own occupancy grid.  Per ray, with weights_sum and the raw depth sum of composite_rays_train over march_rays_train's samples
    (all rays, no jitter; the model's forward under fp16 autocast, as evaluate_views renders): depth = near + raw / weights_sum -- the
    expected distance along the unit ray, given that the ray ended; the training marcher counts a sample's t from the ray's start,
    which without jitter is its near, so the raw sum is sum w (t - near) -- where weights_sum >= min_opacity; +inf (the ray left the
    scene) where weights_sum < free_opacity; NaN (no observation) in between.  The colour is un-premultiplied the same way and 0 elsewhere.
    (The inference branch of render returns a depth clamped and normalised to the slab and not divided by the opacity, and no opacity:
    not this.)  `ray_batch` rays are marched at a time, so an 800 x 800 view needs no more memory than a small one."""
    from .scene import get_rays
    rm = model.rm
    dev = model.aabb_infer.device
    poses = torch.as_tensor(poses, dtype=torch.float32, device=dev)
    V, H, W = int(poses.shape[0]), int(H), int(W)
    intr = torch.as_tensor(intrinsics, dtype=torch.float32).reshape(-1, 4)
    depth = torch.empty(V, H * W, dtype=torch.float32, device=dev)
    opacity = torch.empty(V, H * W, dtype=torch.float32, device=dev)
    color = torch.empty(V, H * W, 3, dtype=torch.float32, device=dev)
    scale = float(model.density_scale)
    for v in range(V):
        rays = get_rays(poses[v:v + 1], tuple(float(x) for x in intr[min(v, intr.shape[0] - 1)]), H, W)
        o, d = rays["rays_o"].reshape(-1, 3).contiguous(), rays["rays_d"].reshape(-1, 3).contiguous()
        for s in range(0, H * W, int(ray_batch)):
            ob, db = o[s:s + int(ray_batch)].contiguous(), d[s:s + int(ray_batch)].contiguous()
            nears, fars = rm.near_far_from_aabb(ob, db, model.aabb_infer, model.min_near)
            xyzs, dirs, deltas, table = rm.march_rays_train(ob, db, model.bound, model.density_bitfield, model.cascade, model.grid_size,
                                                            nears, fars, None, -1, False, 128, True, 0, int(max_steps))
            with torch.autocast("cuda", dtype=torch.float16):
                sigmas, rgbs = model(xyzs, dirs)
            if scale != 1:
                sigmas = scale * sigmas
            ws, wt, img = rm.composite_rays_train(sigmas.float(), rgbs.float(), deltas, table)
            solid, free = ws >= float(min_opacity), ws < float(free_opacity)
            nan = torch.full_like(ws, float("nan"))
            depth[v, s:s + ob.shape[0]] = torch.where(solid, nears + wt / ws, torch.where(free, torch.full_like(ws, float("inf")), nan))
            color[v, s:s + ob.shape[0]] = torch.where(solid[:, None], (img / ws[:, None]).clamp(0.0, 1.0), torch.zeros_like(img))
            opacity[v, s:s + ob.shape[0]] = ws
    return dict(depth=depth.view(V, H, W), color=color.view(V, H, W, 3), opacity=opacity.view(V, H, W))


def extract_surface_tsdf(model, poses=None, intrinsics=None, H=400, W=400, resolution=256, tau=None, bmin=None, bmax=None,
                         views_per_batch=8, min_weight=1.0, unknown=-1.0, min_opacity=0.5, free_opacity=0.05, min_points=0,
                         largest_only=False, normals=True, colors=True, simplify=0, smooth=0, smooth_lambda=0.5, smooth_mu=-0.53,
                         clean=False, min_shell_triangles=0, largest_shell_only=False, texture=0, texture_sh=0, texture_density=0.0,
                         method="tetrahedra"):
    """extract_surface with the geometry taken from what the model RENDERS: depth and colour maps of `poses` (render_depth_maps;
    default tsdf_poses(), with intrinsics of a 50 degree field of view where none are given) are fused into a TSDFVolume over the box
    (default model.aabb_infer), views_per_batch at a time, and the zero level of tsdf_field is meshed -- where the model's rays end,
    whatever its density scale or threshold, with what any camera sees through carved empty.  The dict has extract_surface's shape:
    vertices, triangles, normals (the gradient of the fused field: extract_mesh's with_normals), colors (tsdf_vertex_colors: the
    fused colours, no second pass over the model), field (the TSDF, positive outside), threshold = 0.0 and counts, plus tsdf_totals
    (tsdf_field's) and views.  min_points, largest_only, smooth, simplify, clean, texture and texture_sh mean exactly what they mean in
    extract_surface and go through the same functions, and so do texture_density and method (the mesher of the zero level)."""
    import math
    if method not in MESH_METHODS:
        raise ValueError("method must be one of %s, got %r" % (MESH_METHODS, method))
    aabb = model.aabb_infer
    lo = aabb[:3] if bmin is None else bmin
    hi = aabb[3:] if bmax is None else bmax
    if poses is None:
        poses = tsdf_poses()
    if intrinsics is None:
        focal = 0.5 * W / math.tan(math.radians(25.0))
        intrinsics = (focal, focal, 0.5 * W, 0.5 * H)
    poses = torch.as_tensor(poses, dtype=torch.float32, device=aabb.device)
    intr = torch.as_tensor(intrinsics, dtype=torch.float32).reshape(-1, 4)
    acc = tsdf_volume(resolution, lo, hi, tau=tau, with_color=bool(colors), device=aabb.device)
    step = max(int(views_per_batch), 1)
    for s in range(0, int(poses.shape[0]), step):
        maps = render_depth_maps(model, poses[s:s + step], intr[s:s + step] if intr.shape[0] > 1 else intr, H, W, min_opacity=min_opacity,
                                 free_opacity=free_opacity)
        tsdf_integrate(acc, maps["depth"], poses[s:s + step], intr[s:s + step] if intr.shape[0] > 1 else intr[0],
                       color=maps["color"] if colors else None)
    field, totals = tsdf_field(acc, min_weight=min_weight, unknown=unknown, return_totals=True)
    u = -field  # extract_mesh: inside is u > 0
    counts = None
    if int(min_points) > 0 or largest_only:
        stats, kept = _drop(u, int(resolution), 0.0, min_points, largest_only, u)
        counts = (int(stats[0]),) + tuple(int(v) for v in kept.tolist())
        field = -u
    nrm = col = None
    if normals or colors:
        vertices, triangles, nrm = extract_mesh(u, 0.0, lo, hi, with_normals=True, method=method)
        if colors:
            col = tsdf_vertex_colors(acc, vertices, min_weight=min_weight)
    else:
        vertices, triangles = extract_mesh(u, 0.0, lo, hi, method=method)
    extra = dict(field=field, threshold=0.0, counts=counts, tsdf_totals=totals, views=acc.views)
    return _finish_surface(model, vertices, triangles, nrm, col, normals, lo, hi, extra, smooth, smooth_lambda, smooth_mu, simplify, clean,
                           min_shell_triangles, largest_shell_only, texture, texture_sh, texture_density)


# ------------------------------------------------------------------------------- image projection (csrc/pvd_hip_mesh_project.h)
@torch.no_grad()
def project_views(points, normals, vertices, triangles, color, poses, intrinsics, weight=None, cos_min=0.2, power=2, bias=None,
                  sides="front", mode="blend", min_weight=1e-6, fallback=None, views_per_batch=16, grid=None, _grid=None):
    """dict(colors [N,3] f32 in [0,1], seen [N] bool, weight [N] f32, totals dict(seen, unseen)), device tensors: the colour of every
    surface point (points [N,3] with normals [N,3] of any length) from the posed images color [V,H,W,3] -- poses [V,4,4] cam2world as
    get_rays takes them, intrinsics (fx, fy, cx, cy) for all views or [V,4], weight [V,H,W] optional (a confidence or opacity image; a
    pixel of weight 0 shows nothing).  The standard photogrammetry step: a view counts for a point where it looks at the front of the
    normal (sides="both": at either side) under a cosine above cos_min, the point projects between the centres of the outermost pixels,
    the four pixels around it are finite, and no triangle of the mesh (vertices, triangles) lies between the point -- lifted by `bias`
    along its normal, default 1e-3 of the diagonal of the finite vertices' box -- and the camera: an any-hit walk over mesh_raycast's grid
    with its watertight test (csrc/pvd_hip_mesh_project.h has the definition to the operation; csrc/mesh_project.hip).  mode="blend":
    the views are averaged with the weights cos^power times the bilinear weight; mode="best": the view of the largest weight alone.
    A point whose weight stays below min_weight is unseen and gets `fallback` ([N,3], or a callable (points, unit normals) -> [M,3]
    that is asked for the unseen points only; default 0).  The grid is built once (grid^3 cells, default default_grid(T)) and the views
    are integrated views_per_batch at a time; neither changes a bit of the result.  `weight` in the dict is the accumulated weight.
    Two read-backs: the grid's totals and the two totals of the result.  (_grid: (T, G, pairs, workspace, bias) of an earlier call's
    _project_grid over the same mesh -- view_source builds it once for all the bands of a bake.)"""
    import pvd_hip
    dev = vertices.device
    f = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()  # noqa: E731
    points, normals = f(points).reshape(-1, 3), f(normals).reshape(-1, 3)
    color, poses, weight = f(color), f(poses), f(weight)
    N, V = int(points.shape[0]), int(color.shape[0])
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev)
    if intrinsics.dim() == 1:
        intrinsics = intrinsics[None, :].expand(V, 4)
    intrinsics = intrinsics.contiguous()
    T, G, pairs, ws, bias = _project_grid(vertices, triangles, grid, bias) if _grid is None else _grid
    acc_c = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    acc_w = torch.zeros(N, dtype=torch.float32, device=dev)
    step = max(int(views_per_batch), 1)
    for s in range(0, max(V, 1), step):
        pvd_hip.mesh_project_integrate(points, normals, color[s:s + step], None if weight is None else weight[s:s + step], poses[s:s + step],
                                       intrinsics[s:s + step], T, G, pairs, ws, float(cos_min), int(power), float(bias), sides, mode, acc_c,
                                       acc_w)
    colors = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    if fallback is not None and not callable(fallback):
        colors.copy_(f(fallback).reshape(N, 3))
    seen = torch.empty(N, dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    pvd_hip.mesh_project_finalize(acc_c, acc_w, float(min_weight), mode, colors, seen, totals)
    seen = seen.bool()
    totals = dict(zip(pvd_hip.MESH_PROJECT_TOTALS, (int(x) for x in totals.tolist())))
    if callable(fallback) and totals["unseen"]:
        rest = ~seen
        colors[rest] = fallback(points[rest].contiguous(), _unit_rows(normals[rest]).contiguous()).to(torch.float32).reshape(-1, 3).clamp(0.0, 1.0)
    return dict(colors=colors, seen=seen, weight=acc_w, totals=totals)


def _project_grid(vertices, triangles, grid, bias):
    """(T, G, pairs, workspace, bias): the ray grid of the mesh and the default bias, 1e-3 of the diagonal of the finite vertices' box"""
    vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
    if bias is None:
        lo, hi = _finite_box(vertices)
        diag = float(torch.linalg.norm(hi - lo))
        bias = 1e-3 * diag if diag == diag and diag < float("inf") else 0.0
    return _ray_grid(vertices, triangles, None, None, grid) + (float(bias),)


def _view_fallback(fallback):
    """a model -> its colour head seen straight on (vertex_colors); a callable or None as it is"""
    if fallback is not None and hasattr(fallback, "aabb_infer"):
        model = fallback
        return lambda x, n: vertex_colors(model, x, n)
    return fallback


def view_source(vertices, triangles, color, poses, intrinsics, fallback=None, **kw):
    """A callable (x [M,3], n_unit [M,3]) -> rgb [M,3] for bake_texture: project_views of the images onto the points it is asked for,
    over the mesh (vertices, triangles); kw: project_views' keywords.  fallback: a model (vertex_colors, the colour head seen straight
    on) or a callable (x, n_unit) -> rgb, asked where no view sees the point; without one the colour is 0.
    bake_texture(view_source(...), vertices, triangles, S) bakes the atlas from the images; the ray grid is built here, once."""
    fallback = _view_fallback(fallback)
    built = _project_grid(vertices, triangles, kw.pop("grid", None), kw.pop("bias", None))  # once for every band of the bake

    def source(x, n):
        return project_views(x, n, vertices, triangles, color, poses, intrinsics, fallback=fallback, _grid=built, **kw)["colors"]
    return source


def view_vertex_colors(vertices, triangles, normals, color, poses, intrinsics, fallback=None, **kw):
    """[V,3] f32 in [0,1] on the device: project_views at the vertices with the vertex normals [V,3] (extract_mesh's, or
    face_vertex_normals); fallback and kw as in view_source."""
    return project_views(vertices, normals, vertices, triangles, color, poses, intrinsics, fallback=_view_fallback(fallback), **kw)["colors"]
