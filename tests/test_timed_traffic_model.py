"""Timed fleet traffic without a GPU (mnav_fleet_timed_traffic).

mesh_navigation_amd/csrc/mnav_timed.h compiled for the host (g++ with the library's flags, as tests/test_traffic_model.py
builds its shim: timed_time, timed_slot, timed_window, timed_refusal and -- over fleet_classify -- timed_counts_host are the
device's own source) against tests/timed_traffic_model.py on fields of the oracle: every code, potential bit, cell, holder,
T, peak, window, per-robot report and statistic; a table of edge cases of the window function; the sum over the windows
against tests/traffic_model.py, permutation, accumulation, refusals, zero weights; and the stagger loop, whose per-round
figures are committed below (tests/test_gpu_timed_traffic.py runs the same rounds on the device)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests import fleet_model as FM
from tests import timed_traffic_model as XM
from tests import traffic_model as TM
from tests.fleet_model import bits
from tests.test_dispatch_model import World, _p, mixed_fields, terrain  # noqa: F401  (fixtures: terrain(48) fields of the oracle)
from tests.test_locate_model import CSRC
from tests.test_traffic_model import fleet

SENTINEL = 0xDEADBEEF
F = np.float32
PER_ROBOT = ("conflict_hops", "yield_hops", "first_yield_vertex", "first_yield_window")
WORDS = ("contributing", "adds", "beyond_horizon", "weight", "occupied_cells", "over_cells", "largest_cell", "yielding")   # mnav_timed.h kContributing ...

# The stagger loop: STAGGER_ROBOTS robots of ONE plan (plan 0 of tests/test_gpu_fleet.py's world, offset 1e9), free_count 1,
# 64 windows of tau = the field's largest finite potential / 48, default keys, pace 1; after every round depart[i] += tau
# for the robots with yield_hops[i] > 0.  Per round (over_cells, yielding robots) of tests/timed_traffic_model.py.
STAGGER_ROBOTS, STAGGER_WINDOWS, STAGGER_FREE, STAGGER_ROUNDS = 3000, 64, 1, 6
STAGGER = ((10110, 2915), (10107, 2907), (10105, 2904), (10090, 2903), (10082, 2899), (10072, 2898))

SHIM = r'''
#include <vector>
#include "mnav_timed.h"
using namespace mnav_timed;
extern "C" int timed_counts(uint32_t n, uint32_t V, uint32_t m, const float* dist, const uint32_t* pred, const uint32_t* seed, const uint32_t* target,
                            const double* offset, const uint8_t* on_device, const uint32_t* plan_code, const uint32_t* slot, const uint32_t* vtx,
                            const uint32_t* weights, const float* depart, const float* pace, const uint32_t* key, uint32_t B, double tau,
                            uint32_t free_count, int accumulate, uint32_t state_B, float state_tau, uint32_t* cell, uint32_t* holder,
                            unsigned long long* T, uint32_t* peak, uint32_t* window, uint32_t* code, float* potential, uint32_t* conflict,
                            uint32_t* yield, uint32_t* fy_vertex, uint32_t* fy_window, float* fy_time, unsigned long long* words)
{
  std::vector<Field> fields(m);
  for (uint32_t s = 0; s < m; ++s) {
    Field Fd; Fd.dist = nullptr; Fd.pred = nullptr; Fd.seed = seed[s]; Fd.target = target[s]; Fd.cut = mnav::inf_f(); Fd.code = plan_code[s];
    if (on_device[s]) { Fd.dist = dist + (size_t)V * s; Fd.pred = pred + (size_t)V * s; }
    mnav_fleet::fleet_cut(Fd, offset[s]);
    fields[s] = Fd;
  }
  return timed_counts_host(n, V, fields.data(), slot, vtx, weights, depart, pace, key, B, tau, free_count, accumulate, state_B, state_tau, cell, holder, T,
                           peak, window, code, potential, conflict, yield, fy_vertex, fy_window, fy_time, words);
}
extern "C" void timed_windows(uint32_t m, const float* P, const float* d, const float* depart, const float* pace, const float* tau, const uint32_t* B,
                              uint8_t* inside, uint32_t* k, float* t)
{
  for (uint32_t i = 0; i < m; ++i) {
    k[i] = 0u;
    inside[i] = timed_window(P[i], d[i], depart[i], pace[i], tau[i], B[i], &k[i]) ? 1 : 0;
    t[i] = timed_time(P[i], d[i], depart[i], pace[i]);
  }
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_timed.h"
    d = tmp_path_factory.mktemp("timed_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.timed_counts.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 13 + [C.c_uint32, C.c_double, C.c_uint32, C.c_int, C.c_uint32, C.c_float] + [C.c_void_p] * 13
    L.timed_windows.argtypes = [C.c_uint32] + [C.c_void_p] * 9
    return L


class Mirror:
    """the host mirror's state (cells, holders, their configuration, T, peak, window) over a set of fields"""

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
        self.B, self.tau, self.T = 0, F(0), np.zeros(1, np.uint64)
        self.cell = self.holder = None
        self.peak, self.window = np.zeros(V, np.uint32), np.full(V, FM.NONE, np.uint32)

    def timed(self, slots, vtx, weights=None, depart=None, pace=None, key=None, B=64, tau=1.0, free_count=0, accumulate=False):
        """(rc, dict of the outputs): on rc == -1 every output still holds its sentinel"""
        n = len(slots)
        sl, vt = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
        w, ky = (None if a is None else np.ascontiguousarray(a, np.uint32) for a in (weights, key))
        dp, pc = (None if a is None else np.ascontiguousarray(a, np.float32) for a in (depart, pace))
        keep = self.cell is not None and (accumulate or B == self.B)         # the context reallocates for new windows
        cells = max(self.V * B, 1) if 1 <= B <= XM.MAX_WINDOWS else 1
        cell, holder = (self.cell, self.holder) if keep else (np.full(cells, 77, np.uint32), np.full(cells, 78, np.uint32))
        u = lambda: np.full(n, SENTINEL, np.uint32)
        out = dict(codes=u(), potential=np.full(n, np.nan, F), conflict_hops=u(), yield_hops=u(), first_yield_vertex=u(), first_yield_window=u(),
                   first_yield_time=np.full(n, np.nan, F), words=np.full(len(WORDS), SENTINEL, np.uint64))
        rc = self.L.timed_counts(n, self.V, self.m, _p(self.dist), _p(self.pred), _p(self.seed), _p(self.target), _p(self.offset), _p(self.on), _p(self.pc),
                                 _p(sl), _p(vt), _p(w), _p(dp), _p(pc), _p(ky), B, tau, free_count, 1 if accumulate else 0, self.B if self.cell is not None else 0,
                                 self.tau, _p(cell), _p(holder), _p(self.T), _p(self.peak), _p(self.window), _p(out["codes"]), _p(out["potential"]),
                                 _p(out["conflict_hops"]), _p(out["yield_hops"]), _p(out["first_yield_vertex"]), _p(out["first_yield_window"]),
                                 _p(out["first_yield_time"]), _p(out["words"]))
        if rc == 0:
            self.cell, self.holder, self.B, self.tau = cell, holder, B, np.float64(tau).astype(F)
        elif not keep:
            assert (cell == 77).all() and (holder == 78).all()
        return rc, out

    def snapshot(self):
        return (None if self.cell is None else self.cell.copy(), None if self.holder is None else self.holder.copy(), self.B, self.tau, int(self.T[0]),
                self.peak.copy(), self.window.copy())


def untouched(out):
    return all((out[k] == SENTINEL).all() for k in ("codes",) + PER_ROBOT + ("words",)) and np.isnan(out["potential"]).all() and np.isnan(out["first_yield_time"]).all()


def same_state(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def same(M, state, want, got, where):
    rc, out = got
    assert rc == 0 and want is not None, where
    assert np.array_equal(out["codes"], want["codes"]) and np.array_equal(bits(out["potential"]), bits(want["potential"])), where
    assert np.array_equal(M.cell.reshape(state.V, -1), state.cell), (where, np.argwhere(M.cell.reshape(state.V, -1) != state.cell)[:8])
    assert np.array_equal(M.holder.reshape(state.V, -1), state.holder), where
    assert int(M.T[0]) == state.T == want["total_weight"] and M.B == state.B and M.tau == state.tau, where
    assert np.array_equal(M.peak, state.peak) and np.array_equal(M.window, state.window), where
    for k in PER_ROBOT:
        assert np.array_equal(out[k], want[k]), (where, k, np.flatnonzero(out[k] != want[k])[:8])
    assert np.array_equal(bits(out["first_yield_time"]), bits(want["first_yield_time"])), where
    assert [int(x) for x in out["words"]] == [want[k] for k in WORDS], (where, out["words"], [want[k] for k in WORDS])


def largest_potential(fields):
    return float(max(f.dist[np.isfinite(f.dist)].max() for f in fields if f.dist is not None))


def timing(n, fields, B, seed):
    """random depart, pace and key (duplicates included); tau so that the horizon ends inside the fleet's travel times"""
    rng = np.random.default_rng(seed)
    top = largest_potential(fields)
    depart = (rng.random(n) * 0.2 * top).astype(F)
    pace = (0.5 + rng.random(n)).astype(F)
    key = rng.integers(0, n // 2 + 1, n).astype(np.uint32)
    return depart, pace, key, 0.6 * top / B


_runs = {}


def run_of(W, fields, n):
    """the robots of size n and FM.run over them, computed once"""
    if n not in _runs:
        slots, vtx = fleet(W, fields, n, 300 + n)
        _runs[n] = (slots, vtx, FM.run(fields, W.V, slots, vtx))
    return _runs[n]


@pytest.mark.parametrize("B", [1, 3, 64, 100])
@pytest.mark.parametrize("n", [1, 65, 257, 1200])
def test_host_mirror_equals_the_model(shim, terrain, mixed_fields, n, B):
    W, fields = terrain, mixed_fields
    M, state = Mirror(shim, fields, W.V), XM.Cells(W.V)
    slots, vtx, run = run_of(W, fields, n)
    depart, pace, key, tau = timing(n, fields, B, 7 * n + B)
    for free_count in (2, 0):
        want = XM.timed(state, fields, slots, vtx, None, depart, pace, key, B, tau, free_count, run=run)
        same(M, state, want, M.timed(slots, vtx, None, depart, pace, key, B, tau, free_count), (n, B, free_count))
    if n >= 65:
        assert want["adds"] > 0 and want["beyond_horizon"] > 0, (want["adds"], want["beyond_horizon"])   # both sides of the horizon
        assert 3 * want["contributing"] >= n, want["contributing"]
    if n >= 257:                                                              # free_count 0: cells with two robots, holders that stay, robots that yield
        assert want["over_cells"] > 0 and want["yielding"] > 0 and (want["conflict_hops"] > want["yield_hops"]).any(), (n, B)
    # weights in 0 .. 5 with the default depart, pace and key on top (accumulate), then alone
    w = np.random.default_rng(n).integers(0, 6, n).astype(np.uint32)
    for acc in (True, False):
        want = XM.timed(state, fields, slots, vtx, w, None, None, None, B, tau, 1, accumulate=acc, run=run)
        same(M, state, want, M.timed(slots, vtx, w, B=B, tau=tau, free_count=1, accumulate=acc), (n, B, acc))
    if n >= 257:
        codes = set(int(c) for c in want["codes"])
        assert {FM.SUCCESS, FM.BEYOND_FIELD, FM.NO_PATH_FOUND, FM.INVALID_GOAL, FM.INVALID_START} <= codes, codes


def windows(L, P, d, depart, pace, tau, B):
    a = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, F), np.shape(P)), F) for x in (P, d, depart, pace, tau)]
    Bs = np.ascontiguousarray(np.broadcast_to(np.asarray(B, np.uint32), np.shape(P)), np.uint32)
    m = a[0].size
    inside, k, t = np.full(m, 9, np.uint8), np.full(m, SENTINEL, np.uint32), np.full(m, np.nan, F)
    L.timed_windows(m, *[_p(x) for x in a], _p(Bs), _p(inside), _p(k), _p(t))
    return inside.astype(bool), k, t


def test_window_function_edge_cases(shim):
    inf, below16 = np.inf, np.nextafter(F(16), F(0))
    #        P      d  depart  pace     tau    B    in     k     t
    table = [(6, 0, 0, 1, 2, 8, True, 3, 6),                              # t / tau exactly an integer
             (6, 0, 0, 1, 3, 8, True, 2, 6),
             (16, 0, 0, 1, 2, 8, False, 0, 16),                            # q equal to B: beyond
             (below16, 0, 0, 1, 2, 8, True, 7, below16),                   # ... and just below it
             (0, 0, below16, 1, 2, 8, True, 7, below16),
             (1, 0, 1e9, 1, 1e7, 1024, True, 100, F(1e9)),                 # t absorbs dt
             (1000, 0, 1e9, 1, 1e6, 1024, True, 1000, F(1e9) + F(1000)),   # (the ulp is 64 there: 1000 arrives as 1024)
             (1000, 0, 0, 1e-42, 1e-40, 64, None, None, None),             # a subnormal pace: the model decides
             (3e38, 0, 0, 10, 1, 64, False, 0, inf),                       # P * pace overflows: beyond the horizon
             (3e38, 0, 3e38, 1, 3e38, 64, False, 0, inf),                  # depart + along overflows
             (5, 0, 7, 1, 3e38, 1, True, 0, 12),                           # B = 1 with tau = 3e38: everything finite is window 0
             (3e38, 0, 0, 1, 3e38, 1, False, 0, 3e38),                     # ... but t == tau is not
             (3e38, 0, 0, 2, 3e38, 1, False, 0, inf),
             (2, 5, 4, 1, 1, 64, True, 4, 4),                              # dist[u] above P: dt = 0
             (2, 0, 0, 1, 1, 1024, True, 2, 2),
             (1023.5, 0, 0, 1, 1, 1024, True, 1023, 1023.5),
             (1024, 0, 0, 1, 1, 1024, False, 0, 1024)]
    cols = list(zip(*table))
    inside, k, t = windows(shim, *cols[:6])
    tm = XM.visit_time(*[np.asarray(c, F) for c in cols[:4]])
    for i, row in enumerate(table):
        B, tau = row[5], row[4]
        mi, mk = XM.window_of(tm[i], F(tau), B)
        assert bool(inside[i]) == bool(mi) and bits(t[i]) == bits(tm[i]) and (not mi or k[i] == mk), (row, inside[i], k[i], t[i], mi, mk, tm[i])
        if row[6] is not None:
            assert bool(inside[i]) == row[6] and bits(t[i]) == bits(F(row[8])), (row, inside[i], t[i])
            assert not row[6] or k[i] == row[7], (row, k[i])
    sub = 7
    assert table[sub][3] == 1e-42 and inside[sub] and 0 < t[sub] < np.finfo(F).tiny and k[sub] in (9, 10)     # 1000 * 1e-42 is subnormal
    # random values: the shim against the model, bit for bit
    rng = np.random.default_rng(5)
    m = 20000
    P, d = (rng.random(m) * 100).astype(F), (rng.random(m) * 100).astype(F)
    dp, pc = (rng.random(m) * 30).astype(F), (rng.random(m) * 3 + 1e-3).astype(F)
    tau, B = (rng.random(m) * 4 + 0.01).astype(F), rng.integers(1, 1025, m).astype(np.uint32)
    inside, k, t = windows(shim, P, d, dp, pc, tau, B)
    tm = XM.visit_time(P, d, dp, pc)
    with np.errstate(over="ignore"):
        q = (tm / tau).astype(F)
    mi = q < B.astype(F)
    assert np.array_equal(bits(t), bits(tm)) and np.array_equal(inside, mi) and np.array_equal(k[mi], q[mi].astype(np.uint32)) and 0 < mi.sum() < m


def test_sum_over_the_windows_is_the_untimed_count(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    slots, vtx, run = run_of(W, fields, 1200)
    w = np.random.default_rng(2).integers(0, 6, 1200).astype(np.uint32)
    counts = TM.Counts(W.V)
    TM.traffic(counts, fields, slots, vtx, w)
    depart, pace, key, _ = timing(1200, fields, 64, 1)
    top = largest_potential(fields)
    M, state = Mirror(shim, fields, W.V), XM.Cells(W.V)
    want = XM.timed(state, fields, slots, vtx, w, depart, pace, key, 64, 2.0 * top / 64, run=run)      # a horizon that holds everything
    same(M, state, want, M.timed(slots, vtx, w, depart, pace, key, 64, 2.0 * top / 64), "wide horizon")
    assert want["beyond_horizon"] == 0 and np.array_equal(state.cell.astype(np.uint64).sum(axis=1), counts.c) and state.T == counts.T > 0
    # B = 1 with tau = 3e38: the one window is the count
    want = XM.timed(state, fields, slots, vtx, w, depart, pace, key, 1, 3e38, run=run)
    same(M, state, want, M.timed(slots, vtx, w, depart, pace, key, 1, 3e38), "one window")
    assert want["beyond_horizon"] == 0 and np.array_equal(state.cell[:, 0], counts.c) and np.array_equal(M.peak, counts.c)
    assert np.array_equal(M.window == FM.NONE, counts.c == 0)


def test_permuting_the_robots_with_their_keys_changes_no_cell(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    slots, vtx, _ = run_of(W, fields, 1200)
    depart, pace, key, tau = timing(1200, fields, 64, 3)
    w = np.random.default_rng(8).integers(0, 4, 1200).astype(np.uint32)
    A, Bm = Mirror(shim, fields, W.V), Mirror(shim, fields, W.V)
    rc, a = A.timed(slots, vtx, w, depart, pace, key, 64, tau, 1)
    p = np.random.default_rng(9).permutation(1200)
    rc2, b = Bm.timed(slots[p], vtx[p], w[p], depart[p], pace[p], key[p], 64, tau, 1)
    assert rc == 0 and rc2 == 0 and same_state(A.snapshot(), Bm.snapshot()) and A.cell.max() > 1
    for k in PER_ROBOT:                                                       # ... and every robot gets its own report
        assert np.array_equal(a[k][p], b[k]), k
    assert np.array_equal(bits(a["first_yield_time"][p]), bits(b["first_yield_time"])) and (a["yield_hops"] > 0).any()


def test_accumulating_two_halves_equals_one_call(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    slots, vtx = fleet(W, fields, 600, 9)
    w = np.random.default_rng(4).integers(0, 6, 600).astype(np.uint32)
    depart, pace, key, tau = timing(600, fields, 64, 4)
    whole, halves = Mirror(shim, fields, W.V), Mirror(shim, fields, W.V)
    rc, all_ = whole.timed(slots, vtx, w, depart, pace, key, 64, tau, 1)
    h = slice(0, 251), slice(251, 600)
    rc1, _ = halves.timed(slots[h[0]], vtx[h[0]], w[h[0]], depart[h[0]], pace[h[0]], key[h[0]], 64, tau, 1)
    rc2, second = halves.timed(slots[h[1]], vtx[h[1]], w[h[1]], depart[h[1]], pace[h[1]], key[h[1]], 64, tau, 1, accumulate=True)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and same_state(whole.snapshot(), halves.snapshot()) and whole.cell.max() > 1
    for k in PER_ROBOT:                                                       # the second call's report is taken on all the cells
        assert np.array_equal(all_[k][h[1]], second[k]), k
    state = XM.Cells(W.V)
    XM.timed(state, fields, slots[h[0]], vtx[h[0]], w[h[0]], depart[h[0]], pace[h[0]], key[h[0]], 64, tau, 1)
    XM.timed(state, fields, slots[h[1]], vtx[h[1]], w[h[1]], depart[h[1]], pace[h[1]], key[h[1]], 64, tau, 1, accumulate=True)
    assert np.array_equal(state.cell.ravel(), whole.cell) and np.array_equal(state.holder.ravel(), whole.holder) and state.T == int(whole.T[0])


def test_refusals_touch_nothing(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    M, state = Mirror(shim, fields, W.V), XM.Cells(W.V)
    slots, vtx = fleet(W, fields, 100, 2)
    depart, pace, key, tau = timing(100, fields, 64, 5)
    want = XM.timed(state, fields, slots, vtx, None, depart, pace, key, 64, tau)
    same(M, state, want, M.timed(slots, vtx, None, depart, pace, key, 64, tau), "start")
    snap, cell0, T0 = M.snapshot(), state.cell.copy(), state.T

    def bad(at, value, like):
        a = like.copy()
        a[at] = value
        return a
    two = np.array([2 ** 31, 2 ** 31], np.uint32)
    refusals = [dict(B=0), dict(B=1025), dict(B=2 ** 31), dict(tau=0.0), dict(tau=-1.0), dict(tau=np.nan), dict(tau=np.inf), dict(tau=1e-50), dict(tau=1e39)]
    refusals += [dict(depart=bad(99, x, depart)) for x in (np.nan, -1.0, np.inf, -1e-30)] + [dict(pace=bad(0, x, pace)) for x in (0.0, -1.0, np.nan, np.inf)]
    for kw in refusals:
        for acc in (False, True):
            args = dict(weights=None, depart=depart, pace=pace, key=key, B=64, tau=tau, free_count=0, accumulate=acc)
            args.update(kw)
            rc, out = M.timed(slots, vtx, **args)
            assert rc == -1 and untouched(out) and same_state(M.snapshot(), snap), (kw, acc)
            assert XM.timed(state, fields, slots, vtx, **args) is None and np.array_equal(state.cell, cell0) and state.T == T0, (kw, acc)
    for kw in (dict(B=63), dict(B=1), dict(tau=float(np.nextafter(F(tau), F(0)))), dict(tau=2 * tau)):      # another configuration: only when accumulating
        args = dict(weights=None, depart=depart, pace=pace, key=key, B=64, tau=tau, free_count=0, accumulate=True)
        args.update(kw)
        rc, out = M.timed(slots, vtx, **args)
        assert rc == -1 and untouched(out) and same_state(M.snapshot(), snap), kw
        assert XM.timed(state, fields, slots, vtx, **args) is None and np.array_equal(state.cell, cell0) and state.T == T0, kw
    assert M.timed(slots, vtx, None, depart, pace, key, 64, float(F(tau)) * (1 + 1e-9), accumulate=True)[0] == 0       # the same (float) tau accumulates
    assert XM.timed(state, fields, slots, vtx, None, depart, pace, key, 64, float(F(tau)) * (1 + 1e-9), accumulate=True) is not None
    snap, cell0, T0 = M.snapshot(), state.cell.copy(), state.T
    sl2, vt2 = np.zeros(2, np.uint32), np.array([fields[0].seed, fields[0].target], np.uint32)
    for acc in (False, True):                                                 # the weights that do not fit
        rc, out = M.timed(sl2, vt2, two, B=64, tau=tau, accumulate=acc)
        assert rc == -1 and untouched(out) and same_state(M.snapshot(), snap), acc
        assert XM.timed(state, fields, sl2, vt2, two, B=64, tau=tau, accumulate=acc) is None and np.array_equal(state.cell, cell0) and state.T == T0
    big = np.array([2 ** 32 - 1], np.uint32)                                  # fits when the cells start over, and does not on top of T
    assert M.timed(sl2[:1], vt2[:1], big, B=64, tau=tau, accumulate=True)[0] == -1 and same_state(M.snapshot(), snap)
    rc, out = M.timed(sl2[:1], vt2[:1], big, B=3, tau=tau)
    assert rc == 0 and int(M.T[0]) == 2 ** 32 - 1 == int(M.cell.max()) == int(M.cell[fields[0].seed * 3]) == int(M.peak[fields[0].seed]) and M.B == 3
    assert int(M.holder[fields[0].seed * 3]) == 0 and int(M.window[fields[0].seed]) == 0 and int(out["words"][WORDS.index("largest_cell")]) == 2 ** 32 - 1


def test_zero_weights_are_classified_and_add_nothing(shim, terrain, mixed_fields):
    W, fields = terrain, mixed_fields
    M, state = Mirror(shim, fields, W.V), XM.Cells(W.V)
    slots, vtx = fleet(W, fields, 200, 6)
    zero = np.zeros(200, np.uint32)
    want = XM.timed(state, fields, slots, vtx, zero, B=8, tau=1.0)
    rc, out = M.timed(slots, vtx, zero, B=8, tau=1.0)
    same(M, state, want, (rc, out), "zero weights")
    assert not out["words"].any() and not M.cell.any() and (M.holder == FM.NONE).all() and M.T[0] == 0 and (M.window == FM.NONE).all()
    assert (out["codes"] == FM.SUCCESS).sum() > 50 and not out["conflict_hops"].any() and (out["first_yield_vertex"] == FM.NONE).all() and np.isinf(out["first_yield_time"]).all()


def stagger_world():
    """the one plan of the stagger loop, its robots and its tau: plan 0 of tests/test_gpu_fleet.py's world with the whole field"""
    from tests.test_gpu_fleet import World as GpuWorld
    W = GpuWorld()
    fields = W.fields(offset=1e9)
    vtx = np.random.default_rng(3).integers(0, W.V, STAGGER_ROBOTS).astype(np.uint32)
    tau = float(F(largest_potential(fields[:1]) / 48))
    return W, fields, np.zeros(STAGGER_ROBOTS, np.uint32), vtx, tau


def stagger(call, tau):
    """STAGGER_ROUNDS rounds of call(depart) -> outputs; the robots that yield leave one window later.  Yields every round's outputs."""
    depart = np.zeros(STAGGER_ROBOTS, F)
    for _ in range(STAGGER_ROUNDS):
        out = call(depart)
        yield depart, out
        depart = np.where(out["yield_hops"] > 0, depart + F(tau), depart).astype(F)


def test_stagger_loop(shim):
    W, fields, slots, vtx, tau = stagger_world()
    M, state = Mirror(shim, fields, W.V), XM.Cells(W.V)
    run = FM.run(fields, W.V, slots, vtx)
    seen = []
    for rnd, (depart, out) in enumerate(stagger(lambda d: M.timed(slots, vtx, None, d, B=STAGGER_WINDOWS, tau=tau, free_count=STAGGER_FREE)[1], tau)):
        want = XM.timed(state, fields, slots, vtx, None, depart, B=STAGGER_WINDOWS, tau=tau, free_count=STAGGER_FREE, run=run)
        same(M, state, want, (0, out), ("stagger", rnd))
        seen.append((want["over_cells"], want["yielding"]))
        assert want["beyond_horizon"] == 0 and want["contributing"] > 2900, (rnd, want["beyond_horizon"], want["contributing"])
    print("stagger rounds (over_cells, yielding):", seen)
    assert tuple(seen) == STAGGER, seen
    assert seen[-1][1] < seen[0][1]                                           # fewer robots have to yield after six rounds than at the start
