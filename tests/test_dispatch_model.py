"""Fleet dispatch without a GPU (mnav_fleet_costs, mnav_fleet_assign).

1. The pair rule of tests/dispatch_model.py against tests/fleet_model.py: over fields of OracleMesh.dijkstra, pair() gives
   every vertex the code and the potential of classify(), which walks the chain.
2. mesh_navigation_amd/csrc/mnav_dispatch.h compiled for the host (g++ with the library's flags: dispatch_pair, the keys,
   the quantisation and the bid are the device's own source) against the model, bit for bit: codes, potential bits, both
   nearest arrays, the counters, the assignment, phases, rounds and bids.
3. The auction against an independent exact solver: (size, sum of q) over seeded random problems and spatial ones."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests import dispatch_model as DM
from tests import fleet_model as FM
from tests.fleet_model import bits
from tests.test_locate_model import CSRC

LIMIT = 0.8
OFFSETS = (0.3, -0.2, 1e9)
QUANTUM = 1e-3


class World:
    """a mesh with random costs (some above the limit) and an invalid mask, as in tests/test_fleet_model.py"""

    def __init__(self, mesh):
        self.mesh, self.V = mesh, mesh.V
        self.om = O.OracleMesh(mesh.xyz, mesh.faces)
        rng = np.random.default_rng(11)
        self.costs = rng.random(self.V).astype(np.float32)
        self.invalid = (rng.random(self.V) < 0.03).astype(np.uint8)
        self.w = self.om.edge_weights(self.om.edge_distances(), self.costs, 1.0)
        deg = np.bincount(mesh.faces.ravel(), minlength=self.V)
        self.ok = np.flatnonzero((deg > 0) & (self.costs <= LIMIT) & (self.invalid == 0))

    def field(self, seed, target, offset):
        r = self.om.dijkstra(self.w, self.costs, int(seed), int(target), offset, LIMIT, self.invalid)
        return FM.Field(r.dist, r.pred, int(seed), int(target), offset)


@pytest.fixture(scope="module")
def terrain():
    return World(meshgen.terrain(48, 0.1, 6))


@pytest.fixture(scope="module")
def punched():
    return World(meshgen.punched(48, 0.1, 4, drop=0.12))


@pytest.fixture(scope="module")
def full_fields(terrain):
    """260 full fields (offset 1e9) of the terrain, seeded at distinct vertices: the columns of the spatial problems"""
    rng = np.random.default_rng(21)
    seeds = rng.choice(terrain.ok, 260, replace=False)
    target = int(terrain.ok[0])
    return [terrain.field(s, target if s != target else int(terrain.ok[1]), 1e9) for s in seeds]


@pytest.mark.parametrize("name", ["terrain", "punched"])
def test_pair_rule_equals_the_fleet_rule(name, request):
    W = request.getfixturevalue(name)
    rng = np.random.default_rng(5)
    seen = set()
    for offset in OFFSETS:
        seed, target = (int(x) for x in rng.choice(W.ok, 2, replace=False))
        f = W.field(seed, target, offset)
        codes, pot = DM.matrix([f], W.V, np.arange(W.V + 2))
        for v in range(W.V + 2):
            code, path, p = FM.classify(f, W.V, v)
            got = DM.pair(f, W.V, v)
            assert got[0] == code and bits(got[1]) == bits(p), (name, offset, v, got, code, p)
            assert codes[v, 0] == code and bits(pot[v, 0]) == bits(p), (name, offset, v)
            seen.add(code)
    assert {FM.SUCCESS, FM.BEYOND_FIELD, FM.NO_PATH_FOUND, FM.INVALID_GOAL} <= seen, seen
    assert DM.pair(FM.Field(None, None, 7, 7, 0.3, FM.SUCCESS), W.V, 3) == (FM.SUCCESS, FM.INF)   # seed == target: infeasible by its potential


def test_a_chain_that_misses_the_seed_is_not_detected():
    dist = np.array([0, 1, 2, 3, np.inf, np.inf], np.float32)
    loop = FM.Field(dist, np.array([0, 2, 1, 2, 4, 5], np.uint32), 0, 4, 0.5)
    assert FM.classify(loop, 6, 3)[0] == FM.INTERNAL_ERROR
    assert DM.pair(loop, 6, 3) == (FM.SUCCESS, np.float32(3))              # the one documented difference


# ---------------------------------------------------------------------------------------------------------------------
SHIM = r'''
#include <vector>
#include "mnav_dispatch.h"
using namespace mnav_dispatch;
extern "C" void dispatch_costs(uint32_t n, uint32_t V, uint32_t m, const float* dist, const uint32_t* pred, const uint32_t* seed, const uint32_t* target,
                               const double* offset, const uint8_t* on_device, const uint32_t* plan_code, const uint32_t* vtx, uint8_t* code, float* potential,
                               uint32_t* nearest_slot, uint32_t* nearest_robot, unsigned long long* counters)
{
  std::vector<Field> cols(m);
  for (uint32_t s = 0; s < m; ++s) {
    Field Fd; Fd.dist = nullptr; Fd.pred = nullptr; Fd.seed = seed[s]; Fd.target = target[s]; Fd.cut = mnav::inf_f(); Fd.code = plan_code[s];
    if (on_device[s]) { Fd.dist = dist + (size_t)V * s; Fd.pred = pred + (size_t)V * s; }
    mnav_fleet::fleet_cut(Fd, offset[s]);
    cols[s] = Fd;
  }
  dispatch_costs_host(n, V, m, cols.data(), vtx, code, potential, nearest_slot, nearest_robot, counters);
}
// returns the flag that stopped the auction (0: done), -1: a cost above 2^31 - 1; out[0 .. 3) = phases, rounds, bids
extern "C" int dispatch_assign(uint32_t n, uint32_t m, const uint8_t* code, const float* potential, double quantum, unsigned long long max_rounds, int32_t* q,
                               uint32_t* mine, unsigned long long* out)
{
  const size_t pairs = (size_t)n * m;
  const long long qmax = dispatch_quantise_host(pairs, code, potential, quantum, q);
  if (qmax > kQMax) return -1;
  size_t feasible = 0;
  for (size_t e = 0; e < pairs; ++e) feasible += q[e] >= 0;
  uint32_t phases = 0; unsigned long long rounds = 0, bids = 0;
  const uint32_t flag = dispatch_auction_host(n, m, q, qmax, feasible < pairs, max_rounds, mine, &phases, &rounds, &bids);
  out[0] = phases; out[1] = rounds; out[2] = bids;
  return (int)flag;
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_dispatch.h"
    d = tmp_path_factory.mktemp("dispatch_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.dispatch_costs.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 13
    L.dispatch_assign.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def mirror_costs(L, fields, V, vtx):
    m, n = len(fields), len(vtx)
    dist, pred = np.full((m, V), np.inf, np.float32), np.tile(np.arange(V, dtype=np.uint32), (m, 1))
    on = np.zeros(m, np.uint8)
    for s, f in enumerate(fields):
        if f.dist is not None:
            dist[s], pred[s], on[s] = f.dist, f.pred, 1
    seed, target = (np.array([getattr(f, k) for f in fields], np.uint32) for k in ("seed", "target"))
    offset = np.array([f.offset for f in fields], np.float64)
    pc = np.array([f.code for f in fields], np.uint32)
    vt = np.ascontiguousarray(vtx, np.uint32)
    code, pot = np.full((n, m), 0xEE, np.uint8), np.full((n, m), np.nan, np.float32)
    ns, nr, cnt = np.zeros(n, np.uint32), np.zeros(m, np.uint32), np.zeros(5, np.uint64)
    L.dispatch_costs(n, V, m, _p(dist), _p(pred), _p(seed), _p(target), _p(offset), _p(on), _p(pc), _p(vt), _p(code), _p(pot), _p(ns), _p(nr), _p(cnt))
    return code, pot, ns, nr, [int(c) for c in cnt]


def mirror_assign(L, codes, pot, quantum, max_rounds=1 << 40):
    n, m = codes.shape
    N = max(n, m)
    q, mine, out = np.zeros((n, m), np.int32), np.zeros(N, np.uint32), np.zeros(3, np.uint64)
    flag = L.dispatch_assign(n, m, _p(np.ascontiguousarray(codes)), _p(np.ascontiguousarray(pot)), quantum, max_rounds, _p(q), _p(mine), _p(out))
    return flag, q, mine, [int(x) for x in out]


@pytest.fixture(scope="module")
def mixed_fields(terrain):
    W = terrain
    rng = np.random.default_rng(3)
    fields = []
    for offset in (0.3, -0.2, 1e9, 0.3, 0.6):
        seed, target = (int(x) for x in rng.choice(W.ok, 2, replace=False))
        fields.append(W.field(seed, target, offset))
    fields.append(FM.Field(None, None, W.V + 3, 5, 0.3, FM.INVALID_START))   # plans that never reached the device
    fields.append(FM.Field(None, None, 7, 7, 0.3, FM.SUCCESS))
    return fields


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_host_mirror_equals_the_model(shim, terrain, mixed_fields, n):
    W, fields = terrain, mixed_fields
    rng = np.random.default_rng(100 + n)
    vtx = rng.integers(0, W.V, n).astype(np.uint32)
    if n > 8:
        vtx[:8] = [fields[0].seed, fields[1].target, W.V, FM.NONE, 0, W.V - 1, fields[2].seed, fields[2].seed]
    for cols in (fields, fields[2:3], [fields[i] for i in (4, 0, 6)]):
        codes, pot = DM.matrix(cols, W.V, vtx)
        ns, nr = DM.nearest(codes, pot)
        got = mirror_costs(shim, cols, W.V, vtx)
        assert np.array_equal(got[0], codes) and np.array_equal(bits(got[1]), bits(pot)), (n, len(cols))
        assert np.array_equal(got[2], ns) and np.array_equal(got[3], nr), (n, len(cols))
        assert got[4] == DM.counts(codes) + [int(DM.feasible_of(codes, pot).sum())], (n, got[4])
        if n == 257 and cols is not fields:
            continue                                                        # (the auction at N = 257 once)
        feasible = DM.feasible_of(codes, pot)
        q = DM.quantise(pot, feasible, QUANTUM)
        want = DM.auction(q, feasible)
        flag, q_host, mine, (phases, rounds, bids) = mirror_assign(shim, codes, pot, QUANTUM)
        assert flag == 0 and np.array_equal(q_host, q), (n, flag)
        assert np.array_equal(mine, want["mine"]) and (phases, rounds, bids) == (want["phases"], want["rounds"], want["bids"]), (n, phases, rounds, want["rounds"])
    if n >= 257:
        assert all(c > 0 for c in DM.counts(DM.matrix(fields, W.V, vtx)[0]))      # every outcome occurs


def test_host_mirror_refusals(shim):
    codes, pot = np.zeros((3, 2), np.uint8), np.full((3, 2), 5.0, np.float32)
    assert mirror_assign(shim, codes, pot, 1e-9)[0] == -1                    # 5e9 > 2^31 - 1
    assert mirror_assign(shim, codes, np.arange(6, dtype=np.float32).reshape(3, 2), 1.0, max_rounds=1)[0] == 2   # capped
    assert DM.auction(np.arange(6).reshape(3, 2), np.ones((3, 2), bool), max_rounds=1) is None


# ---------------------------------------------------------------------------------------------------------------------
KINDS = ("random", "identical rows", "all zero", "zero one two", "large")


def random_problem(rng, k):
    """problem k of the optimality test: (q, feasible); kind k % 5 of KINDS with share (k // 5) % 4 of feasible pairs"""
    n, m = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    kind = k % 5
    if kind == 0:
        q = rng.integers(0, 1000, (n, m))
    elif kind == 1:
        q = np.tile(rng.integers(0, 50, (1, m)), (n, 1))                     # identical rows
    elif kind == 2:
        q = np.zeros((n, m), np.int64)                                       # all-zero costs
    elif kind == 3:
        q = rng.integers(0, 3, (n, m))                                       # costs in {0, 1, 2}
    else:
        q = rng.integers(0, 2 ** 20, (n, m))
    share = (0.0, 0.1, 0.5, 1.0)[(k // 5) % 4]
    feasible = rng.random((n, m)) < share if share < 1.0 else np.ones((n, m), bool)
    q = np.where(feasible, q, -1).astype(np.int64)
    return q, feasible


def check_optimal(q, feasible, where):
    a = DM.auction(q, feasible)
    col = a["col_of_robot"]
    got = col[col != FM.NONE]
    assert np.unique(got).size == got.size and all(feasible[i, int(j)] for i, j in enumerate(col) if j != FM.NONE), where
    assert (a["size"], a["total_q"]) == DM.exact(q, feasible), (where, a["size"], a["total_q"], DM.exact(q, feasible))
    return a


@pytest.mark.parametrize("kind", range(5), ids=lambda k: KINDS[k].replace(" ", "_"))
def test_auction_is_optimal_on_random_problems(kind):
    """5 x 44 = 220 seeded problems with 1 <= n, m <= 40: every kind of cost with every share of feasible pairs"""
    rng = np.random.default_rng(2024 + kind)
    shares = set()
    for t in range(44):
        k = 5 * t + kind
        q, feasible = random_problem(rng, k)
        check_optimal(q, feasible, k)
        shares.add((k // 5) % 4)
    assert shares == {0, 1, 2, 3}


def brute_force(q, feasible):
    """(size, total_q) by trying every assignment of a tiny problem"""
    import itertools
    n, m = q.shape
    best = (0, 0)
    for k in range(1, min(n, m) + 1):
        for rows in itertools.combinations(range(n), k):
            for cols in itertools.permutations(range(m), k):
                if all(feasible[i, j] for i, j in zip(rows, cols)):
                    t = sum(int(q[i, j]) for i, j in zip(rows, cols))
                    if k > best[0] or t < best[1]:
                        best = (k, t)
    return best


def test_exact_against_brute_force_and_scipy():
    rng = np.random.default_rng(7)
    for k in range(40):                                                      # tiny problems: every assignment tried
        n, m = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        feasible = rng.random((n, m)) < (0.3, 0.7, 1.0)[k % 3]
        q = np.where(feasible, rng.integers(0, 4 if k % 2 else 100, (n, m)), -1).astype(np.int64)
        assert DM.exact(q, feasible) == brute_force(q, feasible), (k, q)
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        print("scipy does not import here: the brute-force check stands alone")
        return
    for k in range(40):
        q, feasible = random_problem(rng, k)
        cost, N, M = DM.padded(q, feasible)
        r, c = linear_sum_assignment(cost)
        n, m = q.shape
        ok = [(i, j) for i, j in zip(r, c) if i < n and j < m and feasible[i, j]]
        assert DM.exact(q, feasible) == (len(ok), sum(int(q[i, j]) for i, j in ok)), k


def spatial(terrain, full_fields, n, m, seed):
    rng = np.random.default_rng(seed)
    vtx = rng.choice(terrain.ok, n, replace=False)
    codes, pot = DM.matrix(full_fields[:m], terrain.V, vtx)
    feasible = DM.feasible_of(codes, pot)
    return DM.quantise(pot, feasible, QUANTUM), feasible


@pytest.mark.parametrize("n,m", [(130, 257), (257, 130), (64, 64)])
def test_auction_is_optimal_on_spatial_problems(terrain, full_fields, n, m):
    q, feasible = spatial(terrain, full_fields, n, m, n)
    a = check_optimal(q, feasible, (n, m))
    print(n, m, "feasible", int(feasible.sum()), "size", a["size"], "total q", a["total_q"], "phases", a["phases"], "rounds", a["rounds"], "bids", a["bids"])
    assert a["size"] >= min(n, m) // 2
