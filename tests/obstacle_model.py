"""numpy float32 restatement of mnav_layer_obstacle (include/mnav.h; ObstacleLayer::processPointCloud,
obstacle_layer.cpp:216-290): the point filter, the transform, the watertight ray/triangle test of
mesh_navigation_amd/csrc/mnav_ray.h in the same operation order, closest hit with ties to the smallest face id
(brute force over all faces), the lethal set and the change list.  When every ray points straight down the
candidates are culled by a conservative xy binning first."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def ray_setup(d):
    d = np.asarray(d, f32)
    kz = 0
    if abs(d[1]) > abs(d[0]):
        kz = 1
    if abs(d[2]) > abs(d[kz]):
        kz = 2
    kx = 0 if kz + 1 == 3 else kz + 1
    ky = 0 if kx + 1 == 3 else kx + 1
    if d[kz] < 0:
        kx, ky = ky, kx
    with np.errstate(all="ignore"):
        return kx, ky, kz, f32(d[kx] / d[kz]), f32(d[ky] / d[kz]), f32(f32(1.0) / d[kz])


def ray_triangle(setup, o, a, b, c):
    """(n,3) float32 arrays each (o broadcastable) -> (hit bool[n], t float32[n]); t is 0 where there is no hit."""
    kx, ky, kz, sx, sy, sz = setup
    with np.errstate(all="ignore"):
        A = (a - o).astype(f32)
        B = (b - o).astype(f32)
        C = (c - o).astype(f32)
        Ax = A[:, kx] - sx * A[:, kz]; Ay = A[:, ky] - sy * A[:, kz]
        Bx = B[:, kx] - sx * B[:, kz]; By = B[:, ky] - sy * B[:, kz]
        Cx = C[:, kx] - sx * C[:, kz]; Cy = C[:, ky] - sy * C[:, kz]
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        z = (U == 0) | (V == 0) | (W == 0)
        if z.any():
            d = lambda v: v[z].astype(np.float64)
            U[z] = (d(Cx) * d(By) - d(Cy) * d(Bx)).astype(f32)
            V[z] = (d(Ax) * d(Cy) - d(Ay) * d(Cx)).astype(f32)
            W[z] = (d(Bx) * d(Ay) - d(By) * d(Ax)).astype(f32)
        ok = ~(((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0)))
        det = (U + V) + W
        ok &= det != 0
        T = (U * (sz * A[:, kz]) + V * (sz * B[:, kz])) + W * (sz * C[:, kz])
        t = (T / np.where(det == 0, f32(1), det)).astype(f32)
        ok &= t >= 0
    return ok, np.where(ok, t, f32(0)).astype(f32)


def quat_to_matrix(q_wxyz, translation):
    """Eigen::Quaternionf::normalized().toRotationMatrix() (float32) next to the translation: a row-major 3x4."""
    q = np.asarray(q_wxyz, f32)
    w, x, y, z = (q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3], dtype=f32)).astype(f32)
    tx, ty, tz = f32(2) * x, f32(2) * y, f32(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f32(1)
    R = np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                  [txy + twz, one - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, one - (txx + tyy)]], f32)
    return np.concatenate([R, np.asarray(translation, f32).reshape(3, 1)], axis=1).astype(f32)


def keep_and_transform(points, m, max_dist):
    p = np.asarray(points, f32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        n = np.sqrt((x * x + y * y) + z * z, dtype=f32)
        kept = n.astype(np.float64) <= max_dist
        m = np.asarray(m, f32).reshape(3, 4)
        o = np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(f32)
    return kept, o


def _closest(n, ray_idx, face_idx, hit, t):
    """closest hit per ray, ties to the smallest face id: (face int64[n] or -1, t float32[n])"""
    best_t = np.full(n, np.inf, f32)
    r, f, tt = ray_idx[hit], face_idx[hit], t[hit]
    np.minimum.at(best_t, r, tt)
    sel = tt == best_t[r]
    best_f = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(best_f, r[sel], f[sel].astype(np.int64))
    best_f[best_f == np.iinfo(np.int64).max] = -1
    return best_f, best_t


def cast(xyz, faces, origins, d, chunk_pairs=1 << 22):
    """closest-hit face (or -1) and t per ray, brute force over all faces (binned in xy when d = (0,0,-1))"""
    xyz = np.asarray(xyz, f32)
    faces = np.asarray(faces, np.int64)
    o = np.asarray(origins, f32).reshape(-1, 3)
    n, F = o.shape[0], faces.shape[0]
    setup = ray_setup(d)
    best_f = np.full(n, -1, np.int64)
    best_t = np.full(n, np.inf, f32)
    fin = np.isfinite(o).all(axis=1)
    if F == 0 or n == 0:
        return best_f, best_t
    A, B, C = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    d = np.asarray(d, f32)
    down = d[0] == 0 and d[1] == 0 and d[2] < 0
    if down:
        lo = np.minimum(np.minimum(A, B), C)[:, :2].astype(np.float64)
        hi = np.maximum(np.maximum(A, B), C)[:, :2].astype(np.float64)
        pad = 1e-4 * (1.0 + np.abs(np.concatenate([lo, hi], 1)).max(1))[:, None]
        lo, hi = lo - pad, hi + pad
        g0 = lo.min(0)
        cell = max(float(np.median(hi - lo)), 1e-6)
        dims = np.maximum(1, np.ceil((hi.max(0) - g0) / cell).astype(np.int64) + 1)
        c0 = np.floor((lo - g0) / cell).astype(np.int64)
        c1 = np.floor((hi - g0) / cell).astype(np.int64)
        fl, cl = [], []
        for di in range(int((c1[:, 0] - c0[:, 0]).max()) + 1):
            for dj in range(int((c1[:, 1] - c0[:, 1]).max()) + 1):
                m = (c0[:, 0] + di <= c1[:, 0]) & (c0[:, 1] + dj <= c1[:, 1])
                fl.append(np.nonzero(m)[0])
                cl.append((c0[m, 0] + di) * dims[1] + (c0[m, 1] + dj))
        fl, cl = np.concatenate(fl), np.concatenate(cl)
        order = np.argsort(cl, kind="stable")
        fl, cl = fl[order], cl[order]
        ncell = int(dims[0] * dims[1])
        ptr = np.searchsorted(cl, np.arange(ncell + 1))
        rays = np.nonzero(fin)[0]
        ro = o[rays, :2].astype(np.float64)
        ci = np.floor((ro - g0) / cell).astype(np.int64)
        inside = (ci >= 0).all(1) & (ci[:, 0] < dims[0]) & (ci[:, 1] < dims[1])
        rays, ci = rays[inside], ci[inside]
        cid = ci[:, 0] * dims[1] + ci[:, 1]
        cnt = ptr[cid + 1] - ptr[cid]
        ray_idx = np.repeat(rays, cnt)
        start = np.repeat(ptr[cid], cnt)
        off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        face_idx = fl[start + off]
    else:
        rays = np.nonzero(fin)[0]
        ray_idx = np.repeat(rays, F)
        face_idx = np.tile(np.arange(F), rays.size)
    hit_r, hit_f, hit_t = [], [], []
    for s in range(0, ray_idx.size, chunk_pairs):
        r, f = ray_idx[s:s + chunk_pairs], face_idx[s:s + chunk_pairs]
        h, t = ray_triangle(setup, o[r], A[f], B[f], C[f])
        hit_r.append(r[h]); hit_f.append(f[h]); hit_t.append(t[h])
    if hit_r:
        r, f, t = np.concatenate(hit_r), np.concatenate(hit_f), np.concatenate(hit_t)
        bf, bt = _closest(n, r, f, np.ones(r.size, bool), t)
        best_f, best_t = bf, bt
    return best_f, best_t


def obstacle_layer(xyz, faces, points, sensor_to_map=None, down_axis=(0.0, 0.0, -1.0), robot_height=np.inf,
                   max_obstacle_dist=np.inf, old_lethal=None):
    """-> dict(lethal uint8[V], cost float32[V], changed uint32[], kept, hits)"""
    V = np.asarray(xyz).shape[0]
    m = np.eye(3, 4, dtype=f32) if sensor_to_map is None else np.asarray(sensor_to_map, f32).reshape(3, 4)
    kept, o = keep_and_transform(points, m, max_obstacle_dist)
    lethal = np.zeros(V, np.uint8)
    face, t = cast(xyz, faces, o[kept], down_axis)
    hit = face >= 0
    leth = hit & (t.astype(np.float64) <= robot_height)
    lethal[np.asarray(faces, np.int64)[face[leth]].ravel()] = 1
    old = np.zeros(V, np.uint8) if old_lethal is None else np.asarray(old_lethal, np.uint8)
    changed = np.nonzero(lethal != old)[0].astype(np.uint32)
    cost = np.where(lethal == 1, f32(np.inf), f32(0)).astype(f32)
    return dict(lethal=lethal, cost=cost, changed=changed, kept=int(kept.sum()), hits=int(hit.sum()))
