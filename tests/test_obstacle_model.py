"""The obstacle layer's ray/triangle test without a GPU: mesh_navigation_amd/csrc/mnav_ray.h compiled for the host
(g++ -ffp-contract=off, the flags of the library) against tests/obstacle_model.py, its numpy restatement, bit for bit;
the watertight property on shared edges and vertices; the point filter and the robot-height limit at their boundaries."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import obstacle_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mesh_navigation_amd", "csrc")

SHIM = r'''
#include "mnav_ray.h"
using namespace mnav;
extern "C" void cast_pairs(int n, const float* d, const float* o, const float* a, const float* b, const float* c,
                           int* hit, float* t) {
  const RaySetup s = ray_setup(d[0], d[1], d[2]);
  for (int i = 0; i < n; ++i) {
    float tt = 0.f;
    hit[i] = ray_triangle(s, o + 3 * i, a + 3 * i, b + 3 * i, c + 3 * i, &tt);
    t[i] = hit[i] ? tt : 0.f;
  }
}
extern "C" void keep_transform(int n, const float* p, const float* m, double max_dist, int* kept, float* o) {
  for (int i = 0; i < n; ++i) {
    kept[i] = ray_point_kept(p[3 * i], p[3 * i + 1], p[3 * i + 2], max_dist);
    ray_transform(m, p[3 * i], p[3 * i + 1], p[3 * i + 2], o + 3 * i);
  }
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_ray.h"
    d = tmp_path_factory.mktemp("ray_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    vp = C.c_void_p
    L.cast_pairs.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.keep_transform.argtypes = [C.c_int, vp, vp, C.c_double, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_cast(L, d, o, a, b, c):
    n = o.shape[0]
    arrs = [np.ascontiguousarray(x, np.float32) for x in (d, o, a, b, c)]
    hit = np.zeros(n, np.int32)
    t = np.zeros(n, np.float32)
    L.cast_pairs(n, *[_p(x) for x in arrs], _p(hit), _p(t))
    return hit.astype(bool), t


@pytest.mark.parametrize("dir_kind", ["down", "tilted", "random"])
def test_host_routine_equals_the_model_on_random_pairs(shim, dir_kind):
    rng = np.random.default_rng({"down": 1, "tilted": 2, "random": 3}[dir_kind])
    n = 100_000
    if dir_kind == "down":
        d = np.array([0, 0, -1], np.float32)
    elif dir_kind == "tilted":
        d = np.array([0.3, -0.2, -0.93], np.float32)
    else:
        d = rng.normal(size=3).astype(np.float32)
    o = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    a = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    c = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    # edge cases mixed in: degenerate faces, origins on a vertex, on an edge midpoint, exactly on the face plane
    k = n // 20
    b[:k] = a[:k]                                                  # repeated vertex
    o[k:2 * k] = a[k:2 * k] - d * np.float32(0.5)                  # the ray passes through vertex a
    mid = ((a[2 * k:3 * k] + b[2 * k:3 * k]) * np.float32(0.5)).astype(np.float32)
    o[2 * k:3 * k] = mid - d * np.float32(0.25)                    # ... through an edge midpoint
    o[3 * k:4 * k] = a[3 * k:4 * k]                                # origin on the face (t = 0 candidates)
    grid = np.round(rng.uniform(-4, 4, (k, 3, 3))).astype(np.float32) * np.float32(0.25)
    a[4 * k:5 * k], b[4 * k:5 * k], c[4 * k:5 * k] = grid[:, 0], grid[:, 1], grid[:, 2]
    o[4 * k:5 * k] = np.round(rng.uniform(-4, 4, (k, 3))).astype(np.float32) * np.float32(0.25)
    h_host, t_host = host_cast(shim, d, o, a, b, c)
    h_mod, t_mod = M.ray_triangle(M.ray_setup(d), o, a, b, c)
    assert np.array_equal(h_host, h_mod), int((h_host != h_mod).sum())
    assert np.array_equal(t_host.view(np.uint32), t_mod.view(np.uint32))
    assert 0.05 < h_mod.mean() < 0.95
    assert not h_mod[:k].any()                                     # degenerate faces never hit


def _fan(spokes=7, z=0.0):
    ang = np.arange(spokes) * (2 * np.pi / spokes)
    xyz = np.concatenate([[[0.0, 0.0, z]], np.stack([np.cos(ang), np.sin(ang), np.full(spokes, z)], 1)]).astype(np.float32)
    faces = np.array([[0, 1 + s, 1 + (s + 1) % spokes] for s in range(spokes)], np.uint32)
    return xyz, faces


def test_fan_rays_through_shared_vertex_and_edges_hit_the_lowest_face(shim):
    """A ray exactly through the centre vertex or along a shared edge never leaks through: every face touching it that
    the watertight test accepts has the same t here (flat fan, origin at height 1), so the lowest face id wins."""
    xyz, faces = _fan()
    d = np.array([0, 0, -1], np.float32)
    spokes = faces.shape[0]
    origins = [np.array([0, 0, 1], np.float32)]                    # through the shared vertex: all faces touch it
    for s in range(spokes):                                        # through points of the shared edge centre -> spoke s
        for f in (0.25, 0.5):
            p = (xyz[1 + s] * np.float32(f)).astype(np.float32)
            origins.append(np.array([p[0], p[1], 1], np.float32))
    origins = np.stack(origins)
    face, t = M.cast(xyz, faces, origins, d)
    assert (face >= 0).all()                                       # watertight: no ray misses
    A, B, Cc = xyz[faces[:, 0]], xyz[faces[:, 1]], xyz[faces[:, 2]]
    for r in range(origins.shape[0]):
        o = np.repeat(origins[r:r + 1], spokes, 0)
        h, tt = host_cast(shim, d, o, A, B, Cc)
        h2, tt2 = M.ray_triangle(M.ray_setup(d), o, A, B, Cc)
        assert np.array_equal(h, h2) and np.array_equal(tt.view(np.uint32), tt2.view(np.uint32))
        assert h.any()
        assert face[r] == np.nonzero(h)[0].min() and (tt[h] == np.float32(1)).all()
    assert face[0] == 0


def test_filter_transform_and_height_boundaries(shim):
    nan = np.float32(np.nan)
    p = np.array([[3, 4, 0], [3, 4, 0.01], [nan, 0, 0], [0, 0, 0], [1e20, 0, 0], [0, 0, 5]], np.float32)
    m = M.quat_to_matrix([0.9, 0.1, -0.3, 0.2], [1.5, -2.0, 0.25])
    for maxd in (5.0, np.inf, 4.999999):
        kept_h = np.zeros(len(p), np.int32)
        o_h = np.zeros((len(p), 3), np.float32)
        shim.keep_transform(len(p), _p(p), _p(np.ascontiguousarray(m)), maxd, _p(kept_h), _p(o_h))
        kept, o = M.keep_and_transform(p, m, maxd)
        assert np.array_equal(kept_h.astype(bool), kept)
        assert np.array_equal(o_h.view(np.uint32)[np.isfinite(o_h)], o.view(np.uint32)[np.isfinite(o)])
        if maxd == 5.0:
            assert kept.tolist() == [True, False, False, True, False, True]   # norm == max_obstacle_dist is kept, NaN is not
        if maxd == np.inf:
            assert kept.tolist() == [True, True, False, True, True, True]
    # robot height: a hit at t == robot_height is lethal, one ulp above is not
    xyz, faces = _fan()
    pts = np.array([[0.1, 0.05, 2.0]], np.float32)
    for h, want in ((2.0, 1), (np.nextafter(2.0, 0.0), 0), (np.inf, 1)):
        out = M.obstacle_layer(xyz, faces, pts, robot_height=h)
        assert out["hits"] == 1 and int(out["lethal"].sum() > 0) == want, h
    # an empty cloud clears the set and reports every previously lethal vertex
    first = M.obstacle_layer(xyz, faces, pts)
    empty = M.obstacle_layer(xyz, faces, np.zeros((0, 3), np.float32), old_lethal=first["lethal"])
    assert np.array_equal(empty["changed"], np.nonzero(first["lethal"])[0]) and empty["lethal"].sum() == 0


def test_quaternion_matrix_matches_capi():
    from mesh_navigation_amd import capi
    q, t = [0.3, -0.5, 0.7, 0.2], [1.0, 2.0, 3.0]
    a, b = M.quat_to_matrix(q, t), capi.quat_to_matrix(q, t)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    R = a[:, :3].astype(np.float64)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.isclose(np.linalg.det(R), 1.0, atol=1e-6)
