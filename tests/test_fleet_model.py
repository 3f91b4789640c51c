"""Fleet paths without a GPU (mnav_fleet_paths).

The claim: over a field of OracleMesh.dijkstra(seed, target), the rule of tests/fleet_model.py gives every robot it
serves (MNAV_SUCCESS or MNAV_NO_PATH_FOUND) the code, the path and the potential of a fresh OracleMesh.dijkstra(seed, v)
with the same offset, cost_limit and invalid mask, bit for bit; rule 3 (a robot on the seed) gives potential 0 where the
fresh plan clears its maps.  Then mesh_navigation_amd/csrc/mnav_fleet.h compiled for the host (g++ with the library's
flags: fleet_classify and fleet_write are the device's own source, the scan is run block by block as the device runs it)
against the model on the same inputs: codes, lengths, potentials, offsets, packed ids and the outcome counters."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests import fleet_model as FM
from tests.fleet_model import bits
from tests.test_locate_model import CSRC

LIMIT = 0.8
OFFSETS = (0.3, 0.0, -0.2, 1e9)
MESHES = {**{"terrain%d" % s: (lambda s=s: meshgen.terrain(48, 0.1, s)) for s in range(5, 10)},
          "punched": lambda: meshgen.punched(48, 0.1, 4, drop=0.12), "fan": lambda: meshgen.fan_field(spokes=40, rings=6, seed=1)}


class World:
    def __init__(self, name, costs_kind):
        self.name, self.kind = name, costs_kind
        self.mesh = MESHES[name]()
        self.om = O.OracleMesh(self.mesh.xyz, self.mesh.faces)
        self.V = self.mesh.V
        rng = np.random.default_rng(11)
        ed = self.om.edge_distances()
        if costs_kind == "uniform":
            self.costs, self.invalid = np.zeros(self.V, np.float32), None
            self.w = self.om.edge_weights(ed, self.costs, 0.0)
        else:                                                          # random costs, some above the limit, and an invalid mask
            self.costs = rng.random(self.V).astype(np.float32)
            self.invalid = (rng.random(self.V) < 0.03).astype(np.uint8)
            self.w = self.om.edge_weights(ed, self.costs, 1.0)
        deg = np.bincount(self.mesh.faces.ravel(), minlength=self.V)
        ok = (deg > 0) & (self.costs <= LIMIT) & ((self.invalid == 0) if self.invalid is not None else True)
        self.ok = np.flatnonzero(ok)

    def plan(self, seed, target, offset):
        return self.om.dijkstra(self.w, self.costs, seed, target, offset, LIMIT, self.invalid)

    def field(self, seed, target, offset):
        r = self.plan(seed, target, offset)
        return FM.Field(r.dist, r.pred, int(seed), int(target), offset), r


@pytest.fixture(scope="module", params=[(m, k) for m in MESHES for k in ("uniform", "random")], ids=lambda p: "%s-%s" % p)
def world(request):
    return World(*request.param)


def check_claim(W, f, robots, where):
    """every served robot against a fresh plan; returns the counts served / beyond / no path"""
    n = [0, 0, 0]
    for v in robots:
        code, path, pot = FM.classify(f, W.V, int(v))
        if code == FM.BEYOND_FIELD:
            n[1] += 1
            continue
        assert code in (FM.SUCCESS, FM.NO_PATH_FOUND), (where, v, code)
        fresh = W.plan(f.seed, int(v), f.offset)
        assert code == fresh.code, (where, v, code, fresh.code)
        assert np.array_equal(path, fresh.path), (where, v)
        if int(v) == f.seed:
            assert pot == 0 and path.size == 0                          # rule 3 (the fresh plan has cleared its maps by then)
        else:
            assert bits(pot) == bits(fresh.dist[int(v)]), (where, v, pot, fresh.dist[int(v)])
        n[0 if code == FM.SUCCESS else 2] += 1
    return n


def test_the_claim(world):
    W = world
    rng = np.random.default_rng(5)
    seen_unreached_no_path = 0
    for offset in OFFSETS:
        for k in range(2):
            seed, target = (int(x) for x in rng.choice(W.ok, 2, replace=False))
            f, r = W.field(seed, target, offset)
            robots = FM.robots_of(f, W.V, rng, 40)
            served, beyond, no_path = check_claim(W, f, robots, (W.name, W.kind, offset, k))
            print(W.name, W.kind, offset, "served", served, "beyond", beyond, "no path", no_path)
            if offset == 1e9:
                assert beyond == 0, (W.name, W.kind, k)                 # the wave ran out: every robot is served or has no path
                seen_unreached_no_path += no_path
            assert served >= 2                                          # (the seed and the target at least)
    if W.kind == "random" or W.name == "punched":
        assert seen_unreached_no_path > 0, W.name                       # robots on an unreachable component (invalid, or cut off by holes / blocked vertices)


@pytest.mark.parametrize("s", range(5, 10))
def test_a_field_serves_some_robots_and_not_others(s):
    """offset 0.3 on the terrain meshes: a wave from one corner region to the middle covers part of the mesh only"""
    W = World("terrain%d" % s, "uniform")
    rng = np.random.default_rng(s)
    seed, target = W.mesh.vertex_at(0.25, 0.3), W.mesh.vertex_at(0.5, 0.55)
    f, r = W.field(seed, target, 0.3)
    robots = rng.integers(0, W.V, 60)
    served, beyond, no_path = check_claim(W, f, robots, ("condition", s))
    print("terrain", s, "served", served, "beyond", beyond)
    assert served >= 5 and beyond >= 5, (s, served, beyond)


def test_rules_one_to_three_and_broken_chains():
    V = 6
    dist = np.array([0, 1, 2, 3, np.inf, np.inf], np.float32)
    pred = np.array([0, 0, 1, 2, 4, 5], np.uint32)
    f = FM.Field(dist, pred, 0, 2, 0.5)
    assert FM.classify(f, V, V)[0] == FM.INVALID_GOAL and FM.classify(f, V, FM.NONE)[0] == FM.INVALID_GOAL
    assert FM.classify(FM.Field(None, None, 9, 2, 0.5, FM.INVALID_START), V, 1)[0] == FM.INVALID_START
    code, path, pot = FM.classify(f, V, 0)
    assert (code, path.size, float(pot)) == (FM.SUCCESS, 0, 0.0)
    code, path, pot = FM.classify(f, V, 2)
    assert code == FM.SUCCESS and list(path) == [0, 1] and pot == 2
    assert FM.classify(f, V, 3)[0] == FM.BEYOND_FIELD                   # 3 >= cut 2.5: the tentative ring
    assert FM.classify(f, V, 4)[0] == FM.BEYOND_FIELD                   # never reached, but the wave stopped at the cut
    g = FM.Field(dist, pred, 0, 4, 0.5)                                 # the target itself was never reached: the wave ran out
    assert FM.classify(g, V, 4)[0] == FM.NO_PATH_FOUND and FM.classify(g, V, 5)[0] == FM.NO_PATH_FOUND
    assert FM.classify(g, V, 3)[0] == FM.SUCCESS
    h = FM.Field(dist, pred, 0, 3, 0.5)                                 # cut 3.5 above every reached value: the wave ran out under a finite cut
    assert FM.classify(h, V, 4)[0] == FM.NO_PATH_FOUND and FM.classify(h, V, 3)[0] == FM.SUCCESS
    loop = FM.Field(dist, np.array([0, 2, 1, 2, 4, 5], np.uint32), 0, 4, 0.5)   # a chain that never reaches the seed
    assert FM.classify(loop, V, 3)[0] == FM.INTERNAL_ERROR
    assert bits(FM.cut_of(dist, 3, -0.2)) == bits(np.float32(3)) and FM.cut_of(dist, 4, 0.3) == np.inf


# ---------------------------------------------------------------------------------------------------------------------
SHIM = r'''
#include <vector>
#include "mnav_fleet.h"
using namespace mnav_fleet;
// m plans over V vertices (rows of dist / pred; on_device[s] == 0: the plan never ran and code[s] is its own), n robots
extern "C" void fleet_host(uint32_t n, uint32_t V, uint32_t m, const float* dist, const uint32_t* pred, const uint32_t* seed, const uint32_t* target,
                           const double* offset, const uint8_t* on_device, const uint32_t* plan_code, const uint32_t* slot, const uint32_t* vtx, uint32_t* code,
                           uint32_t* len, float* potential, unsigned long long* off, uint32_t* ids, uint32_t* counters)
{
  std::vector<Field> fields(m);
  for (uint32_t s = 0; s < m; ++s) {
    Field Fd; Fd.dist = nullptr; Fd.pred = nullptr; Fd.seed = seed[s]; Fd.target = target[s]; Fd.cut = mnav::inf_f(); Fd.code = plan_code[s];
    if (on_device[s]) { Fd.dist = dist + (size_t)V * s; Fd.pred = pred + (size_t)V * s; }
    fleet_cut(Fd, offset[s]);
    fields[s] = Fd;
  }
  fleet_paths_host(n, V, fields.data(), slot, vtx, code, len, potential, off, ids, counters);
}
extern "C" int fleet_block() { return kFleetBlock; }
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_fleet.h"
    d = tmp_path_factory.mktemp("fleet_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.fleet_host.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 15
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def mirror(L, fields, V, slots, vtx):
    m, n = len(fields), len(slots)
    dist, pred = np.full((m, V), np.inf, np.float32), np.tile(np.arange(V, dtype=np.uint32), (m, 1))
    on = np.zeros(m, np.uint8)
    for s, f in enumerate(fields):
        if f.dist is not None:
            dist[s], pred[s], on[s] = f.dist, f.pred, 1
    seed, target = (np.array([getattr(f, k) for f in fields], np.uint32) for k in ("seed", "target"))
    offset = np.array([f.offset for f in fields], np.float64)
    pc = np.array([f.code for f in fields], np.uint32)
    sl, vt = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
    code, ln, pot, off, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n + 1, np.uint64), np.zeros(4, np.uint32)
    L.fleet_host(n, V, m, _p(dist), _p(pred), _p(seed), _p(target), _p(offset), _p(on), _p(pc), _p(sl), _p(vt), _p(code), _p(ln), _p(pot), _p(off), None, _p(cnt))
    ids = np.full(int(off[n]), 0xDEADBEEF, np.uint32)
    cnt[:] = 0
    L.fleet_host(n, V, m, _p(dist), _p(pred), _p(seed), _p(target), _p(offset), _p(on), _p(pc), _p(sl), _p(vt), _p(code), _p(ln), _p(pot), _p(off), _p(ids), _p(cnt))
    return dict(codes=code, path_len=ln, potential=pot, offsets=off, ids=ids, counts=[int(c) for c in cnt])


def same(got, want, where):
    for k in ("codes", "path_len", "offsets", "ids"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert np.array_equal(bits(got["potential"]), bits(want["potential"])), where
    assert got["counts"] == want["counts"], (where, got["counts"], want["counts"])


@pytest.fixture(scope="module")
def fleet_fields():
    W = World("terrain6", "random")
    rng = np.random.default_rng(3)
    fields = []
    for offset in (0.3, -0.2, 1e9, 0.0):
        seed, target = (int(x) for x in rng.choice(W.ok, 2, replace=False))
        fields.append(W.field(seed, target, offset)[0])
    fields.append(FM.Field(None, None, W.V + 3, 5, 0.3, FM.INVALID_START))   # plans that never reached the device
    fields.append(FM.Field(None, None, 7, 7, 0.3, FM.SUCCESS))
    return W, fields


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 3 * 256 + 41])
def test_host_mirror_equals_the_model(shim, fleet_fields, n):
    assert shim.fleet_block() == FM.BLOCK and 3 * 256 + 41 > 3 * FM.BLOCK     # the largest n spans four blocks of the scan
    W, fields = fleet_fields
    rng = np.random.default_rng(100 + n)
    slots = rng.integers(0, len(fields), n).astype(np.uint32)
    vtx = rng.integers(0, W.V, n).astype(np.uint32)
    if n > 8:
        vtx[:8] = [fields[int(slots[0])].seed, fields[int(slots[1])].target, W.V, FM.NONE, 0, W.V - 1, fields[int(slots[6])].seed, 1]
    want = FM.run(fields, W.V, slots, vtx)
    got = mirror(shim, fields, W.V, slots, vtx)
    same(got, want, n)
    if n >= 257:
        assert all(c > 0 for c in want["counts"]), want["counts"]          # every outcome occurs
        assert int(want["offsets"][n]) == int(want["path_len"].astype(np.uint64).sum()) > 0


def test_host_mirror_with_every_length_zero(shim, fleet_fields):
    W, fields = fleet_fields
    n = 300
    slots = (np.arange(n) % 4).astype(np.uint32)
    vtx = np.array([fields[int(s)].seed for s in slots], np.uint32)     # every robot stands on its plan's seed
    vtx[::3] = W.V + 1                                                   # ... or nowhere
    want = FM.run(fields, W.V, slots, vtx)
    assert int(want["offsets"][n]) == 0 and want["ids"].size == 0
    same(mirror(shim, fields, W.V, slots, vtx), want, "zero")
