"""The clearance and border layers without a GPU: the MNAV_HD rules of mesh_navigation_amd/csrc/mnav_clearance.h compiled
for the host (g++ -ffp-contract=off, the flags of the library) against tests/clearance_model.py bit for bit, and
known answers typed from the reference formulas (clearance_layer.cpp:67-99, border_layer.cpp:66-80)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from tests import clearance_model as M
from tests.clearance_model import up, with_ceiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mesh_navigation_amd", "csrc")
INF = np.float32(np.inf)

SHIM = r'''
#include <stdint.h>
#include <vector>
#include "mnav_build.h"
#include "mnav_clearance.h"
using namespace mnav_clr;
struct Crn { uint32_t v1, v2, ea, eb, ec, face; };
extern "C" void costs(int n, const float* c, double rh, double hi, float* cost, uint8_t* leth) {
  for (int i = 0; i < n; ++i) cost[i] = clr_cost(c[i], rh, hi, leth + i);
}
extern "C" void border_costs(int n, const uint8_t* b, double bc, double th, float* cost, uint8_t* leth) {
  for (int i = 0; i < n; ++i) cost[i] = border_cost_of(b[i] != 0, bc, th, leth + i);
}
extern "C" void borders(uint32_t V, uint32_t F, uint32_t E, const uint32_t* faces, const uint32_t* edges, uint8_t* out) {
  const mnav::HostTopology t = mnav::build_topology(V, F, E, faces, edges);
  std::vector<Crn> crn(t.crn_v1.size());
  for (size_t i = 0; i < crn.size(); ++i) crn[i] = Crn{ t.crn_v1[i], t.crn_v2[i], t.crn_ea[i], t.crn_eb[i], t.crn_ec[i], t.crn_face[i] };
  for (uint32_t v = 0; v < V; ++v)
    out[v] = border_vertex(t.nbr_e.data(), t.row_ptr[v], t.row_ptr[v + 1], crn.data(), t.crn_ptr[v], t.crn_ptr[v + 1]) ? 1 : 0;
}
extern "C" void cast(uint32_t n, const uint32_t* verts, const float* xyz, const float* nrm, const uint32_t* faces, uint32_t F, float* out) {
  for (uint32_t i = 0; i < n; ++i) out[i] = clr_vertex_host(verts[i], xyz, nrm, faces, F, nullptr);
}
extern "C" int rules(uint32_t v, uint32_t a, uint32_t b, uint32_t c, float nx, float ny, float nz) {
  return (clr_excluded(v, a, b, c) ? 1 : 0) | (clr_normal_usable(nx, ny, nz) ? 2 : 0);
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_clearance.h"
    d = tmp_path_factory.mktemp("clearance_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    vp, u32, f64 = C.c_void_p, C.c_uint32, C.c_double
    L.costs.argtypes = [C.c_int, vp, f64, f64, vp, vp]
    L.border_costs.argtypes = [C.c_int, vp, f64, f64, vp, vp]
    L.borders.argtypes = [u32, u32, u32, vp, vp, vp]
    L.cast.argtypes = [u32, vp, vp, vp, vp, u32, vp]
    L.rules.argtypes = [u32, u32, u32, u32, C.c_float, C.c_float, C.c_float]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_costs(L, c, rh, hi):
    c = np.ascontiguousarray(c, np.float32)
    cost, leth = np.zeros(c.size, np.float32), np.zeros(c.size, np.uint8)
    L.costs(c.size, _p(c), rh, hi, _p(cost), _p(leth))
    return cost, leth


def host_border(L, mesh):
    out = np.zeros(mesh.V, np.uint8)
    f, e = np.ascontiguousarray(mesh.faces, np.uint32), np.ascontiguousarray(mesh.edges, np.uint32)
    L.borders(mesh.V, mesh.F, mesh.E, _p(f), _p(e), _p(out))
    return out.astype(bool)


def host_cast(L, xyz, faces, nrm, verts=None):
    xyz, faces, nrm = (np.ascontiguousarray(a, t) for a, t in ((xyz, np.float32), (faces, np.uint32), (nrm, np.float32)))
    verts = np.arange(xyz.shape[0], dtype=np.uint32) if verts is None else np.ascontiguousarray(verts, np.uint32)
    out = np.zeros(verts.size, np.float32)
    L.cast(verts.size, _p(verts), _p(xyz), _p(nrm), _p(faces), faces.shape[0], _p(out))
    return out


def test_cost_rule_equals_the_model_bit_for_bit(shim):
    rng = np.random.default_rng(5)
    for rh, hi in ((0.5, 0.3), (0.25, 1.0), (1.7, 0.05), (0.0, 0.4), (0.5, 0.0)):
        c = np.concatenate([rng.uniform(0, 2.5, 20000), [rh, rh + hi, rh + hi / 2, 0.0, np.inf],
                            np.nextafter(np.float32(rh), np.float32(0)).reshape(1)]).astype(np.float32)
        cost, leth = host_costs(shim, c, rh, hi)
        mc, ml = M.clearance_cost(c, rh, hi)
        assert np.array_equal(bits(cost), bits(mc)) and np.array_equal(leth, ml), (rh, hi)
        assert ((cost > 0) & (cost < 1)).any() or hi == 0.0


def test_cost_known_answers():
    # robot_height 0.5, height_inflation 0.25: every value below is exact in float and in double
    c = np.array([0.5, 0.75, 0.625, np.nextafter(np.float32(0.5), np.float32(0)), 0.0, 0.8, np.inf], np.float32)
    cost, leth = M.clearance_cost(c, 0.5, 0.25)
    assert cost.tolist() == [1.0, 0.0, 0.5, 1.0, 1.0, 0.0, 0.0]      # c == robot_height: cost 1, not lethal; band midpoint: 0.5
    assert leth.tolist() == [0, 0, 0, 1, 1, 0, 0]
    cost, leth = M.clearance_cost(np.array([0.5, 0.5000001], np.float32), 0.5, 0.0)   # no band: cost 0 from robot_height on
    assert cost.tolist() == [0.0, 0.0] and leth.tolist() == [0, 0]


def test_rules(shim):
    assert shim.rules(7, 7, 1, 2, 0, 0, 1) == 3 and shim.rules(7, 1, 2, 3, 0, 0, 1) == 2 and shim.rules(7, 1, 7, 3, 0, 0, 0) == 1
    for n in ((np.nan, 0, 1), (np.inf, 0, 0), (0, 0, 0), (-0.0, 0.0, -0.0)):
        assert shim.rules(0, 1, 2, 3, *n) & 2 == 0 and not M.normal_usable(np.array(n, np.float32)).any()
    assert shim.rules(0, 1, 2, 3, 1e-38, 0, 0) & 2 and M.normal_usable(np.array([1e-38, 0, 0], np.float32)).all()


def test_flat_grid_under_a_ceiling_known_answer(shim):
    ground = meshgen.flat_grid(9, 0.25)
    mesh = with_ceiling(ground, 0.5)
    nrm = up(mesh.V)
    c = M.clearance(mesh.xyz, mesh.faces, nrm)
    assert (c[:ground.V] == np.float32(0.5)).all()                 # every ground vertex, the rim too: watertight
    assert np.isinf(c[ground.V:]).all()                             # nothing above the ceiling
    assert np.array_equal(bits(host_cast(shim, mesh.xyz, mesh.faces, nrm)), bits(c))
    out = M.clearance_layer(c, 0.5, 0.3)
    assert (out["cost"][:ground.V] == 1.0).all() and out["lethal"].sum() == 0
    assert np.array_equal(out["changed"], np.arange(mesh.V))        # a fresh slot: every vertex


@pytest.mark.parametrize("tilt", [False, True])
def test_flat_grid_rays_never_hit_their_own_fan(shim, tilt):
    g = meshgen.flat_grid(16, 0.1)
    xyz, nrm = g.xyz, up(g.V)
    if tilt:
        a, b = 0.05, -0.03
        R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]) @ \
            np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        xyz = (g.xyz.astype(np.float64) @ R.T).astype(np.float32)
        nrm = np.tile((R @ np.array([0.0, 0.0, 1.0])).astype(np.float32), (g.V, 1))
    c = M.clearance(xyz, g.faces, nrm)
    assert np.isinf(c).all()
    assert np.isinf(M.clearance(xyz, g.faces, -nrm)).all()
    assert np.array_equal(bits(host_cast(shim, xyz, g.faces, nrm)), bits(c))


def test_host_cast_equals_the_model_on_terrain_and_sheets(shim):
    from tests import nbhd_model
    ground = meshgen.terrain(24, 0.1, 3, amplitude=0.6)
    for mesh in (with_ceiling(ground, 0.4, step=2, drop=0.2, seed=1), nbhd_model.two_sheets(12, 0.1, 0.2)):
        nrm = M.vertex_normals(mesh.xyz, mesh.faces)
        nrm[::17] = 0.0                                              # a few unusable normals: +inf, no ray
        c, hit = M.clearance_of(mesh.xyz, mesh.faces, nrm)
        assert np.array_equal(bits(host_cast(shim, mesh.xyz, mesh.faces, nrm)), bits(c))
        assert hit.sum() > mesh.V // 10 and np.isinf(c[::17]).all()


def test_coincident_sheets_hit_at_zero():
    g = meshgen.flat_grid(6, 0.5)
    xyz = np.concatenate([g.xyz, g.xyz]).astype(np.float32)
    faces = np.concatenate([g.faces, g.faces + g.V]).astype(np.uint32)
    c = M.clearance(xyz, faces, up(2 * g.V))
    assert (c == 0).all()


def test_border_known_answers(shim):
    tri = meshgen.from_faces(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    assert M.border(3, tri.edges, tri.faces).all() and host_border(shim, tri).all()
    N = 7
    g = meshgen.flat_grid(N, 1.0)
    i, j = np.arange(g.V) % N, np.arange(g.V) // N
    ring = (i == 0) | (j == 0) | (i == N - 1) | (j == N - 1)
    assert np.array_equal(M.border(g.V, g.edges, g.faces), ring) and np.array_equal(host_border(shim, g), ring)
    # punched terrain: an inner grid vertex is a border vertex iff it lost some but not all of its faces; the rim of the
    # grid iff it kept a face; a vertex without faces has no edges and is no border vertex
    P = meshgen.punched(24, 0.1, 3, drop=0.15)
    full = meshgen.terrain(24, 0.1, 3)
    deg_full = np.bincount(full.faces.ravel().astype(np.int64), minlength=full.V)
    deg = np.bincount(P.faces.ravel().astype(np.int64), minlength=P.V)
    i, j = np.arange(P.V) % 24, np.arange(P.V) // 24
    rim = (i == 0) | (j == 0) | (i == 23) | (j == 23)
    want = (deg > 0) & (rim | (deg < deg_full))
    assert want.sum() > 60
    assert np.array_equal(M.border(P.V, P.edges, P.faces), want) and np.array_equal(host_border(shim, P), want)


def test_border_costs(shim):
    b = np.array([1, 0, 1, 0], np.uint8)
    for bc, th, cost, leth in ((1.0, 0.5, [1, 0, 1, 0], [1, 0, 1, 0]), (0.5, 0.5, [0.5, 0, 0.5, 0], [0, 0, 0, 0]),
                               (0.25, -1.0, [0.25, 0, 0.25, 0], [1, 1, 1, 1]), (-2.0, -1.0, [-2, 0, -2, 0], [0, 1, 0, 1])):
        mc, ml = M.border_cost(b, bc, th)
        hc, hl = np.zeros(4, np.float32), np.zeros(4, np.uint8)
        shim.border_costs(4, _p(b), bc, th, _p(hc), _p(hl))
        assert mc.tolist() == cost and ml.tolist() == leth and np.array_equal(bits(hc), bits(mc)) and np.array_equal(hl, ml)


def test_change_list_compares_cost_bits_and_flags():
    c = np.array([0.1, 0.6, 0.9, np.inf], np.float32)
    a = M.clearance_layer(c, 0.5, 0.3)
    b = M.clearance_layer(c, 0.5, 0.5, old_cost=a["cost"], old_lethal=a["lethal"])   # only the band moved
    assert b["changed"].tolist() == [1, 2]
    d = M.clearance_layer(c, 0.05, 0.3, old_cost=b["cost"], old_lethal=b["lethal"])  # vertex 0: cost 1 -> 0.x, flag 1 -> 0
    assert 0 in d["changed"].tolist() and a["lethal"].tolist() == [1, 0, 0, 0]
