"""numpy float32 restatement of mnav_layer_clearance and mnav_layer_border (include/mnav.h; ClearanceLayer,
clearance_layer.cpp:67-99 / :122-164, BorderLayer, border_layer.cpp:66-80 / :104-110).

Clearance: one ray per vertex from p_v along its normal, the watertight test of tests/obstacle_model.py (same operation
order as mesh_navigation_amd/csrc/mnav_ray.h) by brute force over every face without v as a corner, closest hit, +inf
without a hit or a usable normal.  A conservative bounding-sphere cull in double skips faces far from the ray line
first (it cannot drop a face the test hits).  Costs in double with libm's cos (math.cos), stored as float32.  Border:
the edge -> incident-face counts of the uploaded faces (a face side names the first listed edge between its two
vertices, as the library's edge index does).  Both produce the change list against a slot's old costs and flags."""
from __future__ import annotations

import math

import numpy as np

from mesh_navigation_amd import meshgen
from tests import obstacle_model as OM

f32 = np.float32


def vertex_normals(xyz, faces):
    """area-weighted vertex normals in float32 (any normals serve as input: the model uses what it is given)"""
    p = np.asarray(xyz, np.float64)
    f = np.asarray(faces, np.int64)
    fn = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 0
    n[ok] /= ln[ok, None]
    return n.astype(f32)


def normal_usable(n):
    n = np.asarray(n, f32).reshape(-1, 3)
    return np.isfinite(n).all(1) & (n != 0).any(1)


class Faces:
    """per-face corners and bounding spheres (double), shared by the vertices of one cast"""

    def __init__(self, xyz, faces):
        self.xyz = np.asarray(xyz, f32).reshape(-1, 3)
        self.faces = np.asarray(faces, np.int64).reshape(-1, 3)
        A, B, C = (self.xyz[self.faces[:, k]] for k in range(3))
        self.A, self.B, self.C = A, B, C
        a, b, c = (x.astype(np.float64) for x in (A, B, C))
        self.centre = (a + b + c) / 3.0
        r2 = np.maximum(np.maximum(((a - self.centre) ** 2).sum(1), ((b - self.centre) ** 2).sum(1)), ((c - self.centre) ** 2).sum(1))
        m = np.abs(np.concatenate([a, b, c], 1)).max(1) if len(a) else np.zeros(0)
        self.radius = np.sqrt(r2) + 1e-4 * (1.0 + m)                # the BVH leaf padding: far above the test's rounding


def clearance_of(xyz, faces, nrm, verts=None, fc: Faces | None = None):
    """(c float32, hit bool) for v in verts (default: every vertex)"""
    fc = fc or Faces(xyz, faces)
    nrm = np.asarray(nrm, f32).reshape(-1, 3)
    verts = np.arange(fc.xyz.shape[0]) if verts is None else np.asarray(verts, np.int64)
    out = np.full(verts.size, np.inf, f32)
    hit = np.zeros(verts.size, bool)
    usable = normal_usable(nrm[verts])
    for i, v in enumerate(verts):
        if not usable[i] or fc.faces.shape[0] == 0:
            continue
        d, o = nrm[v], fc.xyz[v]
        dd = d.astype(np.float64)
        dn = dd / np.sqrt((dd * dd).sum())
        w = fc.centre - o.astype(np.float64)
        along = w @ dn
        perp2 = np.maximum((w * w).sum(1) - along * along, 0.0)
        cand = (perp2 <= fc.radius * fc.radius * 1.0001 + 1e-12) & (along >= -fc.radius * 1.0001 - 1e-9)
        cand &= (fc.faces != v).all(1)                              # self-exclusion by vertex id
        idx = np.nonzero(cand)[0]
        if idx.size == 0:
            continue
        h, t = OM.ray_triangle(OM.ray_setup(d), o[None, :], fc.A[idx], fc.B[idx], fc.C[idx])
        if h.any():
            out[i] = t[h].min()
            hit[i] = True
    return out, hit


def clearance(xyz, faces, nrm, verts=None):
    return clearance_of(xyz, faces, nrm, verts)[0]


def clearance_cost(c, robot_height, height_inflation):
    """computeLethalsAndCosts (clearance_layer.cpp:77-95): (cost float32, lethal uint8)"""
    c = np.asarray(c, f32).astype(np.float64)
    lethal = (c < robot_height).astype(np.uint8)
    cost = np.zeros(c.shape, f32)
    cost[lethal == 1] = f32(1.0)
    for i in np.nonzero((lethal == 0) & (c < robot_height + height_inflation))[0]:
        diff = (float(c[i]) - robot_height) / height_inflation
        cost[i] = f32((math.cos(diff * math.pi) + 1.0) / 2.0)
    return cost, lethal


def edge_face_counts(edges, faces):
    """incident faces per edge id: a face side names the first listed edge with its two end vertices"""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    key = {}
    for e, (a, b) in enumerate(edges.tolist()):
        key.setdefault((min(a, b), max(a, b)), e)
    cnt = np.zeros(edges.shape[0], np.int64)
    for f in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for k in range(3):
            a, b = f[k], f[(k + 1) % 3]
            cnt[key[(min(a, b), max(a, b))]] += 1
    return cnt


def border(V, edges, faces):
    """bool[V]: v has an edge with fewer than two incident faces"""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    lone = edge_face_counts(edges, faces) < 2
    out = np.zeros(V, bool)
    out[edges[lone, 0]] = True
    out[edges[lone, 1]] = True
    return out


def border_cost(b, border_cost_value, threshold):
    cost = np.where(np.asarray(b, bool), f32(border_cost_value), f32(0)).astype(f32)
    lethal = (cost.astype(np.float64) > threshold).astype(np.uint8)
    return cost, lethal


def changed(cost, lethal, old_cost=None, old_lethal=None):
    """ascending ids whose lethal flag or cost bits differ from the slot's (no old layer: every vertex)"""
    if old_cost is None:
        return np.arange(np.asarray(cost).shape[0], dtype=np.uint32)
    c = np.asarray(cost, f32).view(np.uint32) != np.asarray(old_cost, f32).view(np.uint32)
    return np.nonzero(c | (np.asarray(lethal, np.uint8) != np.asarray(old_lethal, np.uint8)))[0].astype(np.uint32)


def clearance_layer(c, robot_height=0.5, height_inflation=0.3, old_cost=None, old_lethal=None):
    """-> dict(cost, lethal, changed) from the clearance array c"""
    cost, lethal = clearance_cost(c, robot_height, height_inflation)
    return dict(cost=cost, lethal=lethal, changed=changed(cost, lethal, old_cost, old_lethal))


def border_layer(V, edges, faces, border_cost_value=1.0, threshold=0.5, old_cost=None, old_lethal=None):
    b = border(V, edges, faces)
    cost, lethal = border_cost(b, border_cost_value, threshold)
    return dict(border=b, cost=cost, lethal=lethal, changed=changed(cost, lethal, old_cost, old_lethal))


# test geometry
def with_ceiling(ground, z, step=1, drop=0.0, seed=0):
    """ground + a flat sheet at height z over the ground's grid (every `step`-th column / row), faces facing down,
    a `drop` fraction of its faces removed (holes)"""
    n = (ground.N - 1) // step + 1
    g = meshgen.flat_grid(n, ground.h * step)
    top = g.xyz.copy()
    top[:, 2] = z
    faces = g.faces[:, ::-1]
    if drop:
        faces = faces[np.random.default_rng(seed).uniform(size=faces.shape[0]) >= drop]
    xyz = np.concatenate([ground.xyz, top]).astype(np.float32)
    return meshgen.from_faces(xyz, np.concatenate([ground.faces, faces + ground.V]).astype(np.uint32))


def up(V):
    return np.tile(np.array([0, 0, 1], np.float32), (V, 1))
