"""Fleet traffic without a GPU (mnav_fleet_traffic, mnav_layer_traffic).

mesh_navigation_amd/csrc/mnav_traffic.h compiled for the host (g++ with the library's flags, as tests/test_dispatch_model.py
builds its shim: traffic_contributes, traffic_cost and -- over fleet_classify -- traffic_counts_host are the device's own
source) against tests/traffic_model.py on fields of the oracle: every code, potential bit, count, T and statistic; the
accumulate-equals-concatenation property, the overflow refusal, zero weights, and the cost rule bit for bit."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests import fleet_model as FM
from tests import traffic_model as TM
from tests.fleet_model import bits
from tests.test_dispatch_model import World, _p, mixed_fields, terrain  # noqa: F401  (fixtures: terrain(48) fields of the oracle)
from tests.test_locate_model import CSRC

SENTINEL = 0xDEADBEEF

SHIM = r'''
#include <vector>
#include "mnav_traffic.h"
using namespace mnav_traffic;
extern "C" int traffic_counts(uint32_t n, uint32_t V, uint32_t m, const float* dist, const uint32_t* pred, const uint32_t* seed, const uint32_t* target,
                              const double* offset, const uint8_t* on_device, const uint32_t* plan_code, const uint32_t* slot, const uint32_t* vtx,
                              const uint32_t* weights, int accumulate, uint32_t* c, unsigned long long* T, uint32_t* code, float* potential,
                              unsigned long long* sums)
{
  std::vector<Field> fields(m);
  for (uint32_t s = 0; s < m; ++s) {
    Field Fd; Fd.dist = nullptr; Fd.pred = nullptr; Fd.seed = seed[s]; Fd.target = target[s]; Fd.cut = mnav::inf_f(); Fd.code = plan_code[s];
    if (on_device[s]) { Fd.dist = dist + (size_t)V * s; Fd.pred = pred + (size_t)V * s; }
    mnav_fleet::fleet_cut(Fd, offset[s]);
    fields[s] = Fd;
  }
  return traffic_counts_host(n, V, fields.data(), slot, vtx, weights, accumulate, c, T, code, potential, sums);
}
extern "C" void traffic_costs(uint32_t V, const uint32_t* c, uint32_t free_count, double gain, double cap, float* out)
{
  for (uint32_t v = 0; v < V; ++v) out[v] = traffic_cost(c[v], free_count, (float)gain, (float)cap);
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_traffic.h"
    d = tmp_path_factory.mktemp("traffic_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.traffic_counts.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 10 + [C.c_int] + [C.c_void_p] * 5
    L.traffic_costs.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_void_p]
    return L


class Mirror:
    """the host mirror's state (c, T) over a set of fields"""

    def __init__(self, L, fields, V):
        self.L, self.V, self.m = L, V, len(fields)
        self.dist, self.pred = np.full((self.m, V), np.inf, np.float32), np.tile(np.arange(V, dtype=np.uint32), (self.m, 1))
        self.on = np.zeros(self.m, np.uint8)
        for s, f in enumerate(fields):
            if f.dist is not None:
                self.dist[s], self.pred[s], self.on[s] = f.dist, f.pred, 1
        self.seed, self.target = (np.array([getattr(f, k) for f in fields], np.uint32) for k in ("seed", "target"))
        self.offset = np.array([f.offset for f in fields], np.float64)
        self.pc = np.array([f.code for f in fields], np.uint32)
        self.c, self.T = np.zeros(V, np.uint32), np.zeros(1, np.uint64)

    def traffic(self, slots, vtx, weights=None, accumulate=False):
        n = len(slots)
        sl, vt = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint32)
        code, pot, sums = np.full(n, SENTINEL, np.uint32), np.full(n, np.nan, np.float32), np.full(3, SENTINEL, np.uint64)
        rc = self.L.traffic_counts(n, self.V, self.m, _p(self.dist), _p(self.pred), _p(self.seed), _p(self.target), _p(self.offset), _p(self.on), _p(self.pc),
                                   _p(sl), _p(vt), _p(w), 1 if accumulate else 0, _p(self.c), _p(self.T), _p(code), _p(pot), _p(sums))
        return rc, code, pot, [int(x) for x in sums]


def fleet(W, fields, n, seed):
    """n robots over the plans: random vertices, and every plan's seed, target and ids out of range when there is room"""
    rng = np.random.default_rng(seed)
    slots = (np.arange(n) % len(fields)).astype(np.uint32)
    vtx = rng.integers(0, W.V, n).astype(np.uint32)
    if n >= 64:
        k = 0
        for s, f in enumerate(fields):
            special = [f.seed, f.target, W.V, FM.NONE] + ([] if f.dist is None else list(FM.robots_of(f, W.V, rng, 0)))
            for v in special[: max(1, (n // 2) // len(fields))]:
                slots[k], vtx[k] = s, min(int(v), FM.NONE)
                k += 1
    return slots, vtx


def same(M, state, want, got, where):
    rc, code, pot, sums = got
    assert rc == 0 and np.array_equal(code, want["codes"]) and np.array_equal(bits(pot), bits(want["potential"])), where
    assert np.array_equal(M.c, state.c) and int(M.T[0]) == state.T == want["total_weight"], (where, int(M.T[0]), state.T)
    assert sums == [want["contributing"], want["adds"], want["weight"]], (where, sums, want["contributing"], want["adds"], want["weight"])
    assert want["peak"] <= state.T and int(state.c.astype(np.uint64).sum()) >= want["peak"]


@pytest.mark.parametrize("n", [1, 65, 257, 1200])
def test_host_mirror_equals_the_model(shim, terrain, mixed_fields, n):
    W, fields = terrain, mixed_fields
    M, state = Mirror(shim, fields, W.V), TM.Counts(W.V)
    slots, vtx = fleet(W, fields, n, 300 + n)
    want = TM.traffic(state, fields, slots, vtx)
    got = M.traffic(slots, vtx)
    same(M, state, want, got, n)
    assert got[3][2] == want["contributing"]                                 # unit weights: the weight added is the contributors
    assert int(state.c.astype(np.uint64).sum()) == want["adds"]
    # random weights in 0 .. 5 on top (accumulate), then alone
    w = np.random.default_rng(n).integers(0, 6, n).astype(np.uint32)
    for acc in (True, False):
        want = TM.traffic(state, fields, slots, vtx, w, accumulate=acc)
        same(M, state, want, M.traffic(slots, vtx, w, accumulate=acc), (n, acc))
    if n >= 257:
        codes = set(int(c) for c in want["codes"])
        assert {FM.SUCCESS, FM.BEYOND_FIELD, FM.NO_PATH_FOUND, FM.INVALID_GOAL, FM.INVALID_START} <= codes, codes
        on = TM.contributes(want["codes"], want["potential"])
        assert on.sum() >= n // 3 and ((want["codes"] == FM.SUCCESS) & ~on).any()      # the seed == target plan is served and never contributes
        assert want["peak"] > 5 and want["occupied"] > 100


def test_accumulating_two_halves_equals_one_call(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    slots, vtx = fleet(W, fields, 600, 9)
    w = np.random.default_rng(4).integers(0, 6, 600).astype(np.uint32)
    whole, halves = Mirror(shim, fields, W.V), Mirror(shim, fields, W.V)
    halves.c[:] = 77                                                         # accumulate == 0 starts from zero whatever was there
    halves.T[0] = 5
    assert whole.traffic(slots, vtx, w)[0] == 0
    assert halves.traffic(slots[:251], vtx[:251], w[:251])[0] == 0 and halves.traffic(slots[251:], vtx[251:], w[251:], accumulate=True)[0] == 0
    assert np.array_equal(whole.c, halves.c) and whole.T[0] == halves.T[0] and whole.c.max() > 0
    state = TM.Counts(W.V)
    TM.traffic(state, fields, slots[:251], vtx[:251], w[:251])
    TM.traffic(state, fields, slots[251:], vtx[251:], w[251:], accumulate=True)
    assert np.array_equal(state.c, whole.c) and state.T == int(whole.T[0])


def test_weights_that_do_not_fit_are_refused_and_touch_nothing(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    M, state = Mirror(shim, fields, W.V), TM.Counts(W.V)
    slots, vtx = fleet(W, fields, 100, 2)
    TM.traffic(state, fields, slots, vtx)
    assert M.traffic(slots, vtx)[0] == 0 and state.T > 0
    c0, T0 = M.c.copy(), int(M.T[0])
    two = np.array([2 ** 31, 2 ** 31], np.uint32)
    sl2, vt2 = np.zeros(2, np.uint32), np.array([fields[0].seed, fields[0].target], np.uint32)
    for acc in (False, True):
        rc, code, pot, sums = M.traffic(sl2, vt2, two, accumulate=acc)
        assert rc == -1 and (code == SENTINEL).all() and np.isnan(pot).all() and sums == [SENTINEL] * 3
        assert np.array_equal(M.c, c0) and int(M.T[0]) == T0
        assert TM.traffic(state, fields, sl2, vt2, two, accumulate=acc) is None and np.array_equal(state.c, c0) and state.T == T0
    # 2^32 - 1 fits when the counts start over, and does not on top of T
    big = np.array([2 ** 32 - 1], np.uint32)
    assert M.traffic(sl2[:1], vt2[:1], big, accumulate=True)[0] == -1 and np.array_equal(M.c, c0)
    assert M.traffic(sl2[:1], vt2[:1], big)[0] == 0 and int(M.T[0]) == 2 ** 32 - 1 == int(M.c.max()) == int(M.c[fields[0].seed])


def test_zero_weights_are_classified_and_add_nothing(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    M, state = Mirror(shim, fields, W.V), TM.Counts(W.V)
    slots, vtx = fleet(W, fields, 200, 6)
    zero = np.zeros(200, np.uint32)
    want = TM.traffic(state, fields, slots, vtx, zero)
    rc, code, pot, sums = M.traffic(slots, vtx, zero)
    assert rc == 0 and sums == [0, 0, 0] and not M.c.any() and M.T[0] == 0 and want["contributing"] == 0
    assert np.array_equal(code, want["codes"]) and (code == FM.SUCCESS).sum() > 50


def shim_cost(L, c, free_count, gain, cap):
    c = np.ascontiguousarray(c, np.uint32)
    out = np.full(c.size, np.nan, np.float32)
    L.traffic_costs(c.size, _p(c), free_count, gain, cap, _p(out))
    return out


def test_cost_rule(shim):
    c = np.array([0, 1, 2, 3, 7, 8, 9, 100, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 31 + 129, 2 ** 32 - 1], np.uint32)
    for free_count, gain, cap in ((0, 1.0, np.inf), (2, 0.25, 1.5), (0, 0.1, 0.8), (3, 0.0, 5.0), (0, 1.0, 0.0), (2 ** 32 - 1, 3.0, 9.0), (8, 1e30, np.inf),
                                  (1, 1e-40, 1.0), (0, 1 / 3, 1e300), (100, 0.7, 2 ** 24 * 0.7)):
        got, want = shim_cost(shim, c, free_count, gain, cap), TM.cost(c, free_count, gain, cap)
        assert np.array_equal(bits(got), bits(want)), (free_count, gain, cap, got, want)
        assert (got[c <= free_count] == 0).all() and not np.signbit(got).any()
    # e above 2^24: the conversion rounds to nearest even before the multiply
    assert shim_cost(shim, [2 ** 24 + 1, 2 ** 24 + 3], 0, 1.0, np.inf).tolist() == [2.0 ** 24, 2.0 ** 24 + 4]
    assert shim_cost(shim, [2 ** 24 + 11], 10, 0.5, np.inf).tolist() == [2.0 ** 23]
    # the cap hit exactly, from below and above; +inf: no cap; gain 0; free_count >= c
    assert shim_cost(shim, [3, 4, 5], 0, 0.5, 2.0).tolist() == [1.5, 2.0, 2.0]
    assert shim_cost(shim, [2 ** 32 - 1], 0, 3.0e38, np.inf).tolist() == [np.inf]
    assert bits(shim_cost(shim, [1, 50, 2 ** 32 - 1], 0, 0.0, 7.0)).tolist() == [0, 0, 0]
    assert bits(shim_cost(shim, [0, 5, 9], 9, 1.0, 7.0)).tolist() == [0, 0, 0]
    assert shim_cost(shim, [10], 9, 1.0, 7.0).tolist() == [1.0]
