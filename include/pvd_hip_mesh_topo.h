/*
 * pvd_hip_mesh_topo.h -- the topology of a triangle mesh on the device: an edge report (boundary, inconsistent, non-manifold,
 * unbalanced edges), the shells (connected components) and a clean-up that cancels collapsed sheets, drops duplicates and small
 * shells and compacts what is left, in libpvd_hip.so next to the smoothing of pvd_hip_mesh_smooth.h (pvd/mesh.py: mesh_topology,
 * clean_mesh, extract_surface(clean=True)).  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream
 * as void*, PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 *
 * Every quantity below is an integer that does not depend on the order in which anything lands: the results are bit-identical from
 * run to run, and tests/mesh_topo_restatement.py restates them in numpy bit for bit.
 *
 * Inputs   vertices [V,3] f32, triangles [T,3] i32; V and T at most 2^31 - 1.
 *
 * Triangle VALID iff its three indices are in [0, V), its three vertices have finite coordinates, and its three indices are pairwise
 *          different (as in pvd_hip_mesh_smooth.h).  No index is used before it is checked.  Any other triangle is INVALID.
 *
 * Group    the valid triangles with the same vertex set {a < b < c}.  p = the number of them whose corner order is an even
 *          permutation of (a, b, c) (a rotation of it), m = the number whose corner order is an odd one.
 *
 * SURVIVOR of a group: p > m: the lowest-index triangle of even orientation; m > p: the lowest-index triangle of odd orientation;
 *          p == m: none.  The other members of a p != m group are DUPLICATE; all members of a p == m group are CANCELLED (a
 *          collapsed sheet: the same three vertices once in each orientation encloses nothing).  F = the number of survivors.
 *
 * Edge     an undirected pair {a < b} used by at least one survivor.  n_fwd = the survivors that traverse it a -> b, n_bwd = those
 *          that traverse it b -> a.  BOUNDARY: n_fwd + n_bwd == 1.  INCONSISTENT: n_fwd + n_bwd == 2 and n_fwd != 1.  NON-MANIFOLD:
 *          n_fwd + n_bwd >= 3.  UNBALANCED: n_fwd != n_bwd; this overlaps the other classes, and a mesh is closed iff no edge is
 *          unbalanced.
 *
 * Referenced vertex  a corner of a survivor.
 *
 * Shell    survivors are in one shell when they share a vertex, transitively.  A shell's LABEL is its smallest vertex index, its
 *          SIZE its number of survivors.  The LARGEST shell has the most survivors; ties go to the smaller label.
 *
 * Totals   int64 [16]:  0 valid  1 invalid  2 duplicate  3 cancelled  4 survivors F  5 referenced vertices Vr  6 edges E
 *          7 boundary  8 inconsistent  9 non-manifold  10 unbalanced  11 shells  12 the largest shell's size  13 the largest
 *          shell's label (-1 if there is no shell)  14 0  15 0.      valid + invalid == T, duplicate + cancelled + F == valid.
 *          The Euler characteristic Vr - E + F is computed by the caller.
 *
 * Flags    optional, per triangle, u8 [T]: bit0 invalid, bit1 duplicate, bit2 cancelled, bit3 survivor with a boundary edge, bit4
 *          survivor with an inconsistent edge, bit5 survivor with a non-manifold edge.  A survivor has none of bits 0-2.
 *
 * Vertex shell  optional, per vertex, i32 [V]: the label of its shell, -1 when the vertex is not referenced.
 *
 * Clean    with min_shell_triangles >= 0 and largest_only: a triangle is KEPT iff it is a survivor, its shell has at least
 *          min_shell_triangles survivors and, with largest_only, its shell is the largest one.  A vertex is KEPT iff a kept triangle
 *          uses it.  Output vertices: the kept vertices in input order, input bits copied.  Output triangles: the kept triangles in
 *          input order and input corner order, indices remapped.  vertex_map [V] i32 and triangle_map [T] i32: the new index, or -1.
 *          It follows that clean is idempotent (a second application returns the same bits and identity maps), and that the totals
 *          of a mesh cleaned without a shell filter have invalid = duplicate = cancelled = 0 and entries 4-13 unchanged up to the
 *          relabelling of entry 13.
 *
 * Not done No re-orientation of inconsistently wound triangles, no hole filling, no splitting of non-manifold vertices or edges, no
 *          merging of vertices by position: two vertices with the same coordinates and different indices are different vertices.
 *
 * Cost     A triangle is compared with the valid triangles that have the same smallest vertex, an edge with the survivors' edges
 *          that have the same smaller endpoint: linear in T on a mesh of bounded valence, quadratic in the number of triangles that
 *          share one smallest vertex (a fan of n triangles around vertex 0: n^2 comparisons, spread over wavefronts).
 */
#ifndef PVD_HIP_MESH_TOPO_H
#define PVD_HIP_MESH_TOPO_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PVD_MESH_TOPO_TOTALS 16

/* Bytes of workspace for V vertices and T triangles (0 for a V or T outside the limits):
 *     48 V + 45 T + 16 ceil(V / 256) + 4 ceil(T / 256) + 212
 * BUILD'S PART, 8-byte words first: 160 (20 counters: the 16 totals, the packed largest shell, a scan total, two spare) + 8 V (edge
 * counts per smaller endpoint, then the fill cursors) + 8 (V + 1) (edge bucket offsets: up to 3 T entries, which can pass 2^32) +
 * 8 ceil(V / 256) (their per-256 sums) + 24 T (the edge entries: 3 T x (other endpoint | direction, triangle)); then 4 (V + 1) +
 * 4 V + 4 ceil(V / 256) (triangle bucket offsets, cursors, per-256 sums) + 4 T (the triangle buckets) + 4 T (the list of
 * triangles with a long bucket) + 4 V + 4 V + 4 V + 4 V (union-find parents, shell labels, shell sizes, referenced marks) + 4 T (the
 * shell of every survivor, -1 for any other triangle) + 32 (8 words: list lengths, scan totals).
 * CLEAN'S PART: 4 V + 4 (V + 1) + 4 ceil(V / 256) + 4 T + 4 (T + 1) + 4 ceil(T / 256) (keep flags, offsets and per-256 sums of the
 * vertices and of the triangles).  Last, T bytes: the flags of every triangle. */
size_t pvd_mesh_topo_workspace_bytes(uint32_t V, uint32_t T);

/* Computes everything the report needs and leaves it in the workspace: totals_dev int64 [16] on the device, tri_flags [T] u8 and
 * vertex_shell [V] i32 where they are not NULL (the totals are the same either way).  One memset and 18 launches on the stream:
 * per-vertex init; per triangle validity and a count under its smallest vertex; the scan (per-256 sums, one workgroup in chunks,
 * offsets: csrc/block_scan.h); the fill at an atomic cursor per bucket (the order inside a bucket is arbitrary, every predicate is
 * order-free); per triangle its group from its bucket -- a lane for a bucket of at most 64 entries, a wavefront striding by 64 for a
 * longer one, in a launch of its own -- where a survivor counts its three edges under their smaller endpoints, marks its corners
 * and joins them (a union-find by 32-bit integer atomicMin, as csrc/components.hip); the scan of the edge counts, 64-bit; the fill of
 * the edge buckets; per survivor the census of its three edges, lane or wavefront in the same way; the flatten of the union-find;
 * the shell sizes; the largest shell (a packed 64-bit atomicMax); one thread that writes the totals.  No float atomics, no
 * workgroup waits on another one, no retry loop waits for another lane, nothing is read back.
 * V == 0 or T == 0: PVD_OK with totals (0, T, 0, ..., 0, -1, 0, 0) -- every triangle of a mesh without vertices is invalid -- from ONE
 * launch, which also fills tri_flags with bit0 and vertex_shell with -1 where given; vertices, triangles and the workspace are
 * then not used and may be NULL.  Otherwise a NULL vertices, triangles, workspace or totals_dev, a workspace that is not 16-byte
 * aligned or shorter than pvd_mesh_topo_workspace_bytes(V, T): PVD_ERR_INVALID; V or T outside the limits: PVD_ERR_UNSUPPORTED;
 * both before any device call. */
int pvd_mesh_topo_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, void *workspace,
                        size_t workspace_bytes, int64_t *totals_dev, uint8_t *tri_flags, int32_t *vertex_shell, pvd_stream_t stream);

/* counts_dev int64 [2] on the device <- (kept vertices V', kept triangles T') for the filter (min_shell_triangles, largest_only != 0),
 * from what pvd_mesh_topo_build left for the SAME V and T.  It only reads build's part of the workspace and writes clean's part, so
 * different filters can follow one build.  Nine launches: the keep flags of the triangles and of the vertices (from the shells alone:
 * a vertex is kept iff it is referenced and its shell is kept), the two scans (three launches each), the two counts.
 * V == 0 or T == 0: counts (0, 0) from one launch, the workspace is not used.  Argument checks as for pvd_mesh_topo_build. */
int pvd_mesh_topo_clean_count(uint32_t V, uint32_t T, void *workspace, size_t workspace_bytes, uint32_t min_shell_triangles,
                              uint32_t largest_only, int64_t *counts_dev, pvd_stream_t stream);

/* out_vertices [V',3] f32, out_triangles [T',3] i32, vertex_map [V] i32, triangle_map [T] i32 as defined above, for the SAME
 * vertices, triangles and the workspace the last pvd_mesh_topo_clean_count left.  Two launches: one lane per vertex, one per
 * triangle.  out_vertices may be NULL when V' == 0 and out_triangles when T' == 0 (nothing is written through them).  V == 0 or
 * T == 0: both maps are filled with -1 by one launch (none when V == T == 0), nothing else is used.  Argument checks as for
 * pvd_mesh_topo_build; vertex_map NULL with V > 0 or triangle_map NULL with T > 0: PVD_ERR_INVALID. */
int pvd_mesh_topo_clean_emit(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, void *workspace,
                             size_t workspace_bytes, float *out_vertices, int32_t *out_triangles, int32_t *vertex_map,
                             int32_t *triangle_map, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_TOPO_H */
