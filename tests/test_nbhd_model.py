"""The local-neighbourhood layers without a GPU: tests/nbhd_model.py (the numpy restatement the GPU tests compare with)
against a literal lvr2-shaped stack DFS on small meshes, and mesh_navigation_amd/csrc/mnav_nbhd.h compiled for the host
(g++ -ffp-contract=off, the flags of the library) against the model bit for bit: the per-pair rules on random and edge
inputs, and the header's single-threaded routine over whole meshes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests import nbhd_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mesh_navigation_amd", "csrc")
OPS = (M.HEIGHT, M.ROUGH, M.RIDGE)

SHIM = r'''
#include "mnav_nbhd.h"
using namespace mnav_nb;
extern "C" void pairs(int n, const float* pv, const float* nv, const float* pu, const float* nu, double r2,
                      float* d2, int* in, float* rough, float* ridge, long long* frough, long long* fridge) {
  for (int i = 0; i < n; ++i) {
    const float* a = pv + 3 * i; const float* b = pu + 3 * i; const float* na = nv + 3 * i; const float* nb = nu + 3 * i;
    d2[i] = nb_d2(a[0], a[1], a[2], b[0], b[1], b[2]);
    in[i] = nb_in_ball(a[0], a[1], a[2], b[0], b[1], b[2], r2);
    rough[i] = nb_rough_term(na[0], na[1], na[2], nb[0], nb[1], nb[2]);
    ridge[i] = nb_ridge_term(a[0], a[1], a[2], na[0], na[1], na[2], b[0], b[1], b[2], nb[0], nb[1], nb[2]);
    frough[i] = nb_fixed(rough[i]); fridge[i] = nb_fixed(ridge[i]);
  }
}
extern "C" void means(int n, const long long* s, const unsigned* cnt, float* out) {
  for (int i = 0; i < n; ++i) out[i] = nb_mean(s[i], cnt[i]);
}
extern "C" void layer(int op, unsigned V, const unsigned* row_ptr, const unsigned* nbr, const float* xyz, const float* nrm,
                      double r2, unsigned n, const unsigned* centres, float* out, unsigned* size, unsigned* stamp, unsigned* queue) {
  for (unsigned i = 0; i < n; ++i) out[i] = nb_centre_host(op, centres[i], row_ptr, nbr, xyz, nrm, r2, stamp, i + 1, queue, size + i);
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_nbhd.h"
    d = tmp_path_factory.mktemp("nbhd_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    vp = C.c_void_p
    L.pairs.argtypes = [C.c_int, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp]
    L.means.argtypes = [C.c_int, vp, vp, vp]
    L.layer.argtypes = [C.c_int, C.c_uint, vp, vp, vp, vp, C.c_double, C.c_uint, vp, vp, vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_layer(L, op, mesh, nrm, radius, centres=None):
    row_ptr, nbr = M.csr(mesh.V, mesh.edges)
    rp, nb = row_ptr.astype(np.uint32), nbr.astype(np.uint32)
    c = np.arange(mesh.V, dtype=np.uint32) if centres is None else np.asarray(centres, np.uint32)
    out = np.zeros(c.size, np.float32)
    size = np.zeros(c.size, np.uint32)
    stamp = np.zeros(mesh.V, np.uint32)
    queue = np.zeros(mesh.V, np.uint32)
    xyz = np.ascontiguousarray(mesh.xyz, np.float32)
    n3 = np.ascontiguousarray(nrm, np.float32)
    L.layer(OPS.index(op), mesh.V, _p(rp), _p(nb), _p(xyz), _p(n3), float(radius) * float(radius), c.size, _p(c), _p(out), _p(size),
            _p(stamp), _p(queue))
    return out, size


def normals(mesh):
    return O.OracleMesh(mesh.xyz, mesh.faces).vertex_normals()


def meshes():
    return {
        "terrain": meshgen.terrain(30, 0.1, 5),
        "punched": meshgen.punched(36, 0.1, 3, drop=0.15),
        "fan_field": meshgen.fan_field(40, 6, 1),
        "two_sheets": M.two_sheets(16),
    }


@pytest.mark.parametrize("name", ["terrain", "punched", "fan_field", "two_sheets"])
def test_model_equals_the_stack_dfs(name):
    mesh = meshes()[name]
    nrm = normals(mesh)
    row_ptr, nbr = M.csr(mesh.V, mesh.edges)
    rng = np.random.default_rng(11)
    sample = np.unique(np.concatenate([[0, mesh.V - 1], rng.choice(mesh.V, min(mesh.V, 120), replace=False)]))
    for radius in (0.0, 0.25, 0.3):
        for op in OPS:
            val, le, size = M.layer(op, row_ptr, nbr, mesh.xyz, nrm, radius, 0.2, sample)
            for k, v in enumerate(sample):
                want, n = M.dfs_layer(op, row_ptr, nbr, mesh.xyz, nrm, radius, int(v))
                assert size[k] == n, (name, radius, op, v)
                assert np.float32(want).view(np.uint32) == val[k].view(np.uint32), (name, radius, op, v, want, val[k])
            assert np.array_equal(le, (val.astype(np.float64) > 0.2).astype(np.uint8))
            if radius == 0.0:
                assert (size == 1).all()


def test_two_sheets_ball_holds_unreachable_vertices():
    """the reason N(v) is a connected component and not a ball query: the other sheet is 0.2 away, inside the ball"""
    mesh = M.two_sheets(16)
    row_ptr, nbr = M.csr(mesh.V, mesh.edges)
    v = 5 * 16 + 2                                                  # lower sheet, far from the joining strip
    _, _, size = M.layer(M.HEIGHT, row_ptr, nbr, mesh.xyz, None, 0.3, 0.1, [v])
    ball = int(M.in_ball(mesh.xyz[v], mesh.xyz, 0.3).sum())
    assert ball > size[0] > 1
    val, _, _ = M.layer(M.HEIGHT, row_ptr, nbr, mesh.xyz, None, 0.3, 0.1, [v])
    assert val[0] == 0.0                                            # only its own flat sheet


def test_exact_boundary_is_excluded():
    mesh = M.exact_boundary(8)
    row_ptr, nbr = M.csr(mesh.V, mesh.edges)
    _, _, size = M.layer(M.HEIGHT, row_ptr, nbr, mesh.xyz, None, 0.5, 0.1)
    assert (size == 1).all()                                        # grid neighbours at d2 == r*r exactly: outside
    _, _, size = M.layer(M.HEIGHT, row_ptr, nbr, mesh.xyz, None, 0.75, 0.1)
    assert size.max() >= 5 and size.min() >= 3


def test_pair_rules_equal_the_model(shim):
    rng = np.random.default_rng(5)
    n = 200_000
    pv = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    pu = (pv + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
    nv = rng.normal(size=(n, 3)).astype(np.float32)
    nv /= np.linalg.norm(nv, axis=1, keepdims=True)
    nu = (nv + rng.normal(0, 0.4, (n, 3))).astype(np.float32)
    nu /= np.linalg.norm(nu, axis=1, keepdims=True)
    nv, nu = nv.astype(np.float32), nu.astype(np.float32)
    k = n // 10
    nu[:k] = nv[:k]                                                 # dot(n, n) of a unit normal: may round above 1
    nu[k:2 * k] = -nv[k:2 * k]                                      # ... or below -1
    nu[2 * k:2 * k + 100] = 0.0                                     # a zero normal
    nv[2 * k + 100:2 * k + 200] = 0.0
    nu[3 * k:4 * k] = (nv[3 * k:4 * k] * np.float32(1.01)).astype(np.float32)   # |dot| > 1 for certain
    pu[4 * k:5 * k], nu[4 * k:5 * k] = pv[4 * k:5 * k], nv[4 * k:5 * k]      # u == v: ridge term 0
    r = 0.5
    pv[5 * k:6 * k] = np.round(pv[5 * k:6 * k] * 8) / 8                       # d2 == r*r exactly (sums of eighths are exact)
    pu[5 * k:6 * k] = pv[5 * k:6 * k] + np.array([r, 0, 0], np.float32)
    d2 = np.zeros(n, np.float32)
    inb = np.zeros(n, np.int32)
    rough = np.zeros(n, np.float32)
    ridge = np.zeros(n, np.float32)
    fr = np.zeros(n, np.int64)
    fd = np.zeros(n, np.int64)
    shim.pairs(n, _p(pv), _p(nv), _p(pu), _p(nu), r * r, _p(d2), _p(inb), _p(rough), _p(ridge), _p(fr), _p(fd))
    assert np.array_equal(d2.view(np.uint32), M.d2(pv, pu).view(np.uint32))
    assert np.array_equal(inb.astype(bool), M.in_ball(pv, pu, r))
    assert not inb[5 * k:6 * k].any() and (d2[5 * k:6 * k] == np.float32(r * r)).all()
    mr = M.rough_term(nv, nu)
    assert np.array_equal(rough.view(np.uint32), mr.view(np.uint32))
    assert np.isfinite(mr).all() and (mr[3 * k:4 * k] == 0.0).all()
    assert (mr[2 * k:2 * k + 200] == M.acosf(np.float32(0.0))).all()
    md = M.ridge_term(pv, nv, pu, nu)
    assert np.array_equal(ridge.view(np.uint32), md.view(np.uint32))
    assert (md[4 * k:5 * k] == 0.0).all()
    assert np.array_equal(fr, M.fixed(mr)) and np.array_equal(fd, M.fixed(md))
    # the mean, including sums near 2^63 and ties of the fixed-point rounding
    s = np.concatenate([rng.integers(0, 2 ** 62, 1000), [0, 1, 2 ** 31, 2 ** 63 - 1]]).astype(np.int64)
    cnt = np.concatenate([rng.integers(1, 5000, 1000), [1, 3, 7, 1]]).astype(np.uint32)
    out = np.zeros(s.size, np.float32)
    shim.means(s.size, _p(s), _p(cnt), _p(out))
    assert np.array_equal(out.view(np.uint32), M.mean(s, cnt).view(np.uint32))
    half = np.array([0.5, 1.5, 2.5, -0.5], np.float64) / M.FIX        # t * 2^32 = k + 0.5: half to even
    assert list(M.fixed(half.astype(np.float32))) == [0, 2, 2, 0]


@pytest.mark.parametrize("name", ["terrain", "punched", "fan_field", "two_sheets"])
def test_header_routine_equals_the_model(shim, name):
    mesh = meshes()[name]
    nrm = normals(mesh)
    row_ptr, nbr = M.csr(mesh.V, mesh.edges)
    for radius in (0.0, 0.3, 1.0, 50.0):
        for op in OPS:
            want, _, size = M.layer(op, row_ptr, nbr, mesh.xyz, nrm, radius, 0.3)
            got, gsize = host_layer(shim, op, mesh, nrm, radius)
            assert np.array_equal(gsize, size), (name, radius, op)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, radius, op)
