"""The device rollout without a GPU: mesh_navigation_amd/csrc/mnav_rollout.h compiled for the host (g++
-ffp-contract=off, the flags of the library) -- rol_after_tick is the device's own source, rol_run composes it with
mnav_follow.h's fol_tick serially -- against tests/rollout_model.py, the Python restatement of the specification with the
host libm's cosf, sinf and acosf.  Every comparison is exact (floats and doubles by their bits; any NaN equals any NaN),
and the trace at stride 1 pins every tick, not only the end.  Also: chunk invariance of rol_run, stopped robots, the
block loop's look at the cancel flag, and the fold of a call's counter rows into its statistics (rol_fold_counters)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests import follow_model as FM
from tests import rollout_model as RM
from tests.test_follow_model import CONFIGS, MESHES, build_world
from tests.test_locate_model import CSRC, SHIM as LOCATE_SHIM

SHIM = LOCATE_SHIM + r'''
#include <cstring>
#include "mnav_rollout.h"
using mnav_rol::State;

// the state of robot i as the arrays hold it, and back
struct Rows { int32_t* status; uint32_t* ticks; float* pos; float* dir; const float* up; uint32_t* face; double* travel; double* cost_integral; float* min_goal_dist; };
static State load(const Rows& A, uint32_t i)
{
  State S;
  S.pos = mnav::w3_load(A.pos + 3 * (size_t)i); S.dir = mnav::w3_load(A.dir + 3 * (size_t)i); S.up = mnav::w3_load(A.up + 3 * (size_t)i);
  S.face = A.face[i]; S.status = A.status[i]; S.ticks = A.ticks[i]; S.travel = A.travel[i]; S.cost_integral = A.cost_integral[i];
  S.min_goal_dist = A.min_goal_dist[i];
  return S;
}
static void store(const Rows& A, uint32_t i, const State& S)
{
  A.pos[3 * (size_t)i] = S.pos.x; A.pos[3 * (size_t)i + 1] = S.pos.y; A.pos[3 * (size_t)i + 2] = S.pos.z;
  A.dir[3 * (size_t)i] = S.dir.x; A.dir[3 * (size_t)i + 1] = S.dir.y; A.dir[3 * (size_t)i + 2] = S.dir.z;
  A.face[i] = S.face; A.status[i] = S.status; A.ticks[i] = S.ticks; A.travel[i] = S.travel; A.cost_integral[i] = S.cost_integral;
  A.min_goal_dist[i] = S.min_goal_dist;
}
static mnav_rol::Params params(const double* par, bool have_goal) { return mnav_rol::Params{ par[0], (float)par[1], (float)par[2], have_goal }; }

// n robots through rol_run from the state the rows hold; fields: S vector maps of V rows each; par = dt, dist_tolerance,
// angle_tolerance; seed_face / goal_pos (with goal_dir) / trace may be null; how: 5 counters
extern "C" void rol_batch(void* h, uint32_t n, const uint32_t* slot, const uint32_t* seed_face, const float* goal_pos, const float* goal_dir, const float* fields,
                          const float* costs, const double* cfg, const double* par, uint32_t ticks, uint32_t stride, uint32_t V, uint32_t F, const float* xyz,
                          const uint32_t* faces, const uint32_t* vf_ptr, const uint32_t* vf, int32_t* status, uint32_t* tk, float* pos, float* dir,
                          const float* up, uint32_t* face, double* travel, double* cost_integral, float* min_goal_dist, float* trace, uint64_t* how)
{
  Host* H = (Host*)h;
  const Index I{ H->nodes.data(), H->pts.data(), H->n_pts, H->n_leaves, loc_root(H->n_leaves) };
  const mnav::WalkMesh Mh{ xyz, faces, vf_ptr, vf, V, F };
  mnav_fol::Config Cf;
  std::memcpy(&Cf, cfg, sizeof(Cf));
  const mnav_rol::Params P = params(par, goal_pos != nullptr);
  const Rows A{ status, tk, pos, dir, up, face, travel, cost_integral, min_goal_dist };
  VecStack st; st.cap = kStack;
  std::vector<uint32_t> list(mnav::kWalkScratchWords);
  const uint32_t rows = stride ? ticks / stride : 0;
  for (uint32_t i = 0; i < n; ++i) {
    const mnav::WalkField Fd = mnav_fol::fol_field(Mh, fields + 3 * (size_t)V * slot[i], seed_face ? seed_face[i] : mnav::kNone);
    State S = load(A, i);
    const mnav::W3 zero = mnav::w3(0, 0, 0);
    mnav_rol::rol_run(Mh, I, st, Fd, costs, Cf, P, goal_pos ? mnav::w3_load(goal_pos + 3 * (size_t)i) : zero, goal_dir ? mnav::w3_load(goal_dir + 3 * (size_t)i) : zero,
                      S, ticks, stride, trace ? trace + 3 * (size_t)rows * i : nullptr, list.data(), how);
    store(A, i, S);
  }
}
// rol_after_tick on every RUNNING row, the tick's result taken from the outputs of one mnav_follow_batch call
extern "C" void rol_after(uint32_t n, const float* goal_pos, const float* goal_dir, const double* par, const int32_t* code, const int32_t* how, const uint32_t* face_r,
                          const float* pos_r, const float* cost, const double* cmd, int32_t* status, uint32_t* tk, float* pos, float* dir, const float* up,
                          uint32_t* face, double* travel, double* cost_integral, float* min_goal_dist)
{
  const mnav_rol::Params P = params(par, goal_pos != nullptr);
  const Rows A{ status, tk, pos, dir, up, face, travel, cost_integral, min_goal_dist };
  for (uint32_t i = 0; i < n; ++i) {
    State S = load(A, i);
    if (S.status != mnav_rol::kRunning) continue;
    mnav_fol::Result R = mnav_fol::fol_lost(S.pos);
    R.code = code[i]; R.how = how[i]; R.face = face_r[i]; R.pos = mnav::w3_load(pos_r + 3 * (size_t)i); R.cost = cost[i]; R.lin = cmd[2 * (size_t)i]; R.ang = cmd[2 * (size_t)i + 1];
    const mnav::W3 zero = mnav::w3(0, 0, 0);
    mnav_rol::rol_after_tick(S, R, P, goal_pos ? mnav::w3_load(goal_pos + 3 * (size_t)i) : zero, goal_dir ? mnav::w3_load(goal_dir + 3 * (size_t)i) : zero);
    store(A, i, S);
  }
}
// the block loop of the call with a flag that is found set at look number cancel_at (0: never); blocks[2 * k], [2 * k + 1] =
// first tick and length of block k
extern "C" int rol_block_loop(uint32_t ticks, uint32_t cancel_at, int fail_at, uint32_t* blocks, uint32_t* n_blocks, uint32_t* looks, uint32_t* done)
{
  *n_blocks = 0; *looks = 0;
  return mnav_rol::rol_blocks(ticks,
                              [&](uint32_t first, uint32_t nt) { blocks[2 * *n_blocks] = first; blocks[2 * *n_blocks + 1] = nt; ++*n_blocks; return (int)*n_blocks == fail_at ? -1 : 0; },
                              [&] { return ++*looks == cancel_at; }, done);
}
// rol_fold_counters over `ticks` counter rows of a call of n robots; out: the four final statuses, robot_ticks, stayed,
// neighbour, global, and what the fold must leave alone: built_index, ms_kernels, ms_total
extern "C" void rol_fold(const uint32_t* cnt, uint32_t ticks, uint32_t n, uint64_t* out)
{
  mnav_rol::Stats S;
  mnav_rol::rol_fold_counters(cnt, ticks, n, S);
  for (int k = 0; k < 4; ++k) out[k] = S.final_status[k];
  out[4] = S.robot_ticks; out[5] = S.stayed; out[6] = S.neighbour; out[7] = S.global;
  out[8] = S.built_index; out[9] = S.ms_kernels != 0.f; out[10] = S.ms_total != 0.f;
}
'''


def build_shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_rollout.h"
    d = tmp_path_factory.mktemp("rollout_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    vp, u32 = C.c_void_p, C.c_uint32
    L.loc_build.restype = vp
    L.loc_build.argtypes = [u32, vp]
    L.loc_free.argtypes = [vp]
    L.rol_batch.argtypes = [vp, u32] + [vp] * 8 + [u32] * 4 + [vp] * 15
    L.rol_after.argtypes = [u32] + [vp] * 18
    L.rol_block_loop.restype = C.c_int
    L.rol_block_loop.argtypes = [u32, u32, C.c_int] + [vp] * 4
    L.rol_fold.argtypes = [vp, u32, u32, vp]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fresh_state(robots):
    """the rows of n robots before their first tick"""
    n = robots["pos"].shape[0]
    return dict(status=np.zeros(n, np.int32), ticks=np.zeros(n, np.uint32), pos=np.array(robots["pos"], np.float32), dir=np.array(robots["dir"], np.float32),
                face=np.array(robots["face_in"], np.uint32), travel=np.zeros(n, np.float64), cost_integral=np.zeros(n, np.float64),
                min_goal_dist=np.full(n, np.inf, np.float32))


def _goal(goals, k):
    return None if goals is None else np.ascontiguousarray(goals[k], np.float32)


class Mirror:
    """mnav_rollout.h on the host over one mesh"""

    def __init__(self, L, model):
        self.L, self.m = L, model
        self.h = L.loc_build(model.V, _p(model.xyz))
        self.ptr, self.vf = np.ascontiguousarray(model.ptr, np.uint32), np.ascontiguousarray(model.vf, np.uint32)

    def close(self):
        self.L.loc_free(self.h)

    def run(self, cfg, fields, robots, goals, dt, ticks, dist_tol=0.0, ang_tol=0.0, trace_stride=0, state=None):
        """rol_run for every robot, from `state` (the dict a previous run returned) or from the start; returns the rows,
        the trace and the ticks by `how`"""
        m = self.m
        n = robots["pos"].shape[0]
        S = fresh_state(robots) if state is None else {k: state[k].copy() for k in RM.KEYS}
        fl = np.ascontiguousarray(np.stack(fields), np.float32)
        c = np.array([cfg[k] for k in FM.CFG_NAMES], np.float64)
        par = np.array([dt, dist_tol, ang_tol], np.float64)
        up, slot = np.ascontiguousarray(robots["up"], np.float32), np.ascontiguousarray(robots["slot"], np.uint32)
        sf = None if robots.get("seed_face") is None else np.ascontiguousarray(robots["seed_face"], np.uint32)
        gp, gd = _goal(goals, 0), _goal(goals, 1)
        trace = np.zeros((n, ticks // trace_stride, 3), np.float32) if trace_stride else None
        how = np.zeros(5, np.uint64)
        self.L.rol_batch(self.h, n, _p(slot), _p(sf), _p(gp), _p(gd), _p(fl), _p(m.costs), _p(c), _p(par), ticks, trace_stride, m.V, m.F, _p(m.xyz),
                         _p(m.faces), _p(self.ptr), _p(self.vf), _p(S["status"]), _p(S["ticks"]), _p(S["pos"]), _p(S["dir"]), _p(up), _p(S["face"]),
                         _p(S["travel"]), _p(S["cost_integral"]), _p(S["min_goal_dist"]), _p(trace), _p(how))
        return dict(S, trace=trace, how=how.astype(np.int64))


def after_tick(L, S, up, goals, dt, dist_tol, ang_tol, tick_out):
    """rol_after_tick (the header's own) on the rows S, in place, with the outputs of one follower call"""
    par = np.array([dt, dist_tol, ang_tol], np.float64)
    o = {k: np.ascontiguousarray(tick_out[k]) for k in ("code", "how", "face", "pos", "cost", "cmd")}
    L.rol_after(S["pos"].shape[0], _p(_goal(goals, 0)), _p(_goal(goals, 1)), _p(par), _p(o["code"]), _p(o["how"]), _p(o["face"]), _p(o["pos"]), _p(o["cost"]),
                _p(o["cmd"]), _p(S["status"]), _p(S["ticks"]), _p(S["pos"]), _p(S["dir"]), _p(np.ascontiguousarray(up, np.float32)), _p(S["face"]),
                _p(S["travel"]), _p(S["cost_integral"]), _p(S["min_goal_dist"]))


def fleet(model, n_slots, seed_faces, seed, per_family, drivers, close=5):
    """robots of every family of follow_model.make_robots (those beside the mesh leave the map, those on the outer part
    have no field) plus `drivers` around the mesh's middle, where every field points, on their face or with none yet:
    the first `close` of them start a short way west of the middle and head for it, the others on a wider ring with any
    heading.  A goal per robot, heading +x: the middle of the mesh, or for every fourth robot (on every plan in turn) a
    point far off the mesh, which it never reaches: it keeps circling where its field ends, or runs out of field"""
    robots, _ = FM.make_robots(model, n_slots, seed_faces, seed, per_family=per_family)
    rng = np.random.default_rng(seed + 1)
    cen = model.xyz[model.faces].astype(np.float64).mean(axis=1)
    mid = np.nanmean(cen, axis=0)
    r = np.linalg.norm(cen[:, :2] - mid[None, :2], axis=1)
    lo, hi = np.nanquantile(r, [0.04, 0.3])
    near = np.nonzero((r > 0.45) & (r < 0.9) & (cen[:, 0] < mid[0] - 0.3))[0]
    f = np.concatenate([rng.choice(near, close), rng.choice(np.nonzero((r > lo) & (r < hi))[0], drivers - close)])
    pos = FM.face_points(model, f, rng)
    a = rng.uniform(0, 2 * np.pi, drivers)
    d = np.stack([np.cos(a), np.sin(a), np.zeros(drivers)], axis=1)
    to_mid = (mid - pos) * np.array([1, 1, 0])
    to_mid /= np.linalg.norm(to_mid, axis=1, keepdims=True)
    d[:close] = to_mid[:close]
    up = np.tile(np.array([0, 0, 1], np.float32), (drivers, 1))
    face_in = np.where(np.arange(drivers) % 3 == 0, FM.NONE, f)
    slot = (np.arange(drivers) % n_slots).astype(np.uint32)
    extra = dict(pos=pos.astype(np.float32), dir=d.astype(np.float32), up=up, face_in=face_in.astype(np.uint32), slot=slot,
                 seed_face=np.asarray(seed_faces, np.uint32)[slot])
    n0 = robots["pos"].shape[0]
    robots = {k: np.concatenate([robots[k], extra[k]]) for k in robots}
    n = robots["pos"].shape[0]
    goal_pos = np.tile(cen[int(np.nanargmin(r))].astype(np.float32), (n, 1))
    far = np.arange(n) % 4 == 3
    far[n0:n0 + close] = False
    goal_pos[far, 0] += 50.0
    return robots, (goal_pos, np.tile(np.array([1, 0, 0], np.float32), (n, 1)))


DT, TICKS, DIST_TOL, ANG_TOL = 0.25, 120, 0.4, 2.0
FLEET_SEED = {"terrain": 40, "holes": 42, "hub": 42}      # seeds at which the model's outcomes meet assert_every_outcome with every config


@pytest.fixture(scope="module", params=list(MESHES))
def world(request, shim):
    mesh, model, fields, seed_faces, start_face = build_world(request.param)
    mirror = Mirror(shim, model)
    robots, goals = fleet(model, len(fields), seed_faces, FLEET_SEED[request.param], per_family=1, drivers=15)
    assert robots["pos"].shape[0] <= 24
    yield request.param, model, fields, robots, goals, mirror
    mirror.close()


@pytest.mark.parametrize("cfg_name,with_goals,with_seeds", [(c, g, s) for c in ("default", "saturating") for g in (True, False) for s in (True, False)])
def test_rol_run_equals_the_model(world, cfg_name, with_goals, with_seeds):
    name, model, fields, robots, goals, mirror = world
    cfg = CONFIGS[cfg_name]
    r = robots if with_seeds else dict(robots, seed_face=None)
    g = goals if with_goals else None
    want = RM.run(model, cfg, fields, r, g, DT, TICKS, DIST_TOL, ANG_TOL, trace_stride=1)
    got = mirror.run(cfg, fields, r, g, DT, TICKS, DIST_TOL, ANG_TOL, trace_stride=1)
    print(name, cfg_name, with_goals, with_seeds, "status:", np.bincount(want["status"], minlength=4), "how:", want["how"], "ticks:", want["ticks"])
    RM.assert_same(got, want, (name, cfg_name, with_goals, with_seeds))
    assert np.array_equal(got["how"], want["how"])
    if with_goals:
        RM.assert_every_outcome(want, (name, cfg_name, with_seeds))
        assert np.isfinite(want["min_goal_dist"]).any()
    else:
        assert set(want["status"].tolist()) == {RM.RUNNING, RM.OUT_OF_MAP, RM.NO_FIELD} and np.isinf(want["min_goal_dist"]).all()
        assert want["how"][1] > 0 and want["how"][2] > 0 and want["how"][3] > 0


def test_chunks_and_stopped_robots(world):
    name, model, fields, robots, goals, mirror = world
    cfg = CONFIGS["default"]
    whole = mirror.run(cfg, fields, robots, goals, DT, TICKS, DIST_TOL, ANG_TOL, trace_stride=1)
    a = mirror.run(cfg, fields, robots, goals, DT, 50, DIST_TOL, ANG_TOL, trace_stride=1)
    b = mirror.run(cfg, fields, robots, goals, DT, 70, DIST_TOL, ANG_TOL, trace_stride=1, state=a)
    RM.assert_same(b, whole, (name, "50 + 70"), keys=RM.KEYS)
    assert FM.same_bits(np.concatenate([a["trace"], b["trace"]], axis=1), whole["trace"])
    assert np.array_equal(a["how"] + b["how"], whole["how"])
    # a stopped robot is left untouched: the rows of the robots that had stopped after 50 ticks are the final ones
    stopped = a["status"] != RM.RUNNING
    assert stopped.any() and not stopped.all()
    RM.assert_same({k: a[k][stopped] for k in RM.KEYS}, {k: whole[k][stopped] for k in RM.KEYS}, (name, "stopped"), keys=RM.KEYS)
    assert FM.same_bits(whole["trace"][stopped, 50:], np.repeat(whole["trace"][stopped, 49:50], TICKS - 50, axis=1))   # ... and its trace row repeats
    # the trace at another stride is the stride-1 trace thinned out (120 % 7 != 0: the last ticks leave no row)
    t7 = mirror.run(cfg, fields, robots, goals, DT, TICKS, DIST_TOL, ANG_TOL, trace_stride=7)
    assert t7["trace"].shape[1] == TICKS // 7 and FM.same_bits(t7["trace"], whole["trace"][:, 6::7][:, : TICKS // 7])
    RM.assert_same(t7, whole, (name, "stride 7"), keys=RM.KEYS)


def test_the_block_loop_looks_at_the_flag_once_per_block(shim):
    def loop(ticks, cancel_at=0, fail_at=0):
        blocks, nb, looks, done = np.zeros(2 * 512, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        rc = shim.rol_block_loop(ticks, cancel_at, fail_at, _p(blocks), _p(nb), _p(looks), _p(done))
        return rc, blocks[: 2 * int(nb[0])].reshape(-1, 2).tolist(), int(looks[0]), int(done[0])

    assert loop(1) == (0, [[0, 1]], 1, 1)
    assert loop(256) == (0, [[0, 256]], 1, 256)
    assert loop(300) == (0, [[0, 256], [256, 44]], 2, 300)
    assert loop(100000)[1][-1] == [99840, 160] and loop(100000)[2:] == (391, 100000)
    # a flag found at the first look ends the call after one block: 1, and the ticks run so far
    assert loop(300, cancel_at=1) == (1, [[0, 256]], 1, 256)
    assert loop(1000, cancel_at=3) == (1, [[0, 256], [256, 256], [512, 256]], 3, 768)
    assert loop(300, cancel_at=2) == (1, [[0, 256], [256, 44]], 2, 300)   # after the last block: still "cancelled"
    # an error of a block is passed on, nothing more is started and the flag is not looked at
    assert loop(1000, fail_at=2) == (-1, [[0, 256], [256, 256]], 1, 256)


def test_the_counter_rows_fold_into_the_statistics(shim):
    """a counter table written by hand in which every statistic is another number; words 0 and 1 of a row (the work lists'
    lengths) tell nothing"""
    cnt = np.array([[9999, 77777, 1, 20, 300, 4000, 50000, 600000],
                    [123, 456, 2, 30, 400, 5000, 60000, 700000],
                    [7, 8, 4, 40, 500, 6000, 70000, 800000]], np.uint32)
    names = ("running", "reached", "out_of_map", "no_field", "robot_ticks", "stayed", "neighbour", "global", "built_index", "ms_kernels", "ms_total")

    def fold(ticks, n):
        out = np.full(len(names), 99, np.uint64)
        shim.rol_fold(_p(cnt), ticks, n, _p(out))
        return dict(zip(names, out.tolist()))

    stopped = 15000 + 180000 + 2100000
    want = dict(running=13, reached=15000, out_of_map=180000, no_field=2100000, robot_ticks=7 + 90 + 1200 + 180000, stayed=7, neighbour=90,
                **{"global": 1200}, built_index=0, ms_kernels=0, ms_total=0)
    assert fold(3, stopped + 13) == want and len(set(list(want.values())[:8])) == 8
    assert fold(3, stopped)["running"] == 0
    # a cancelled call folds the rows of the ticks it ran
    assert fold(2, 2000000) == dict(want, running=2000000 - (9000 + 110000 + 1300000), reached=9000, out_of_map=110000, no_field=1300000,
                                    robot_ticks=3 + 50 + 700 + 110000, stayed=3, neighbour=50, **{"global": 700})
    assert fold(0, 5) == dict(want, running=5, reached=0, out_of_map=0, no_field=0, robot_ticks=0, stayed=0, neighbour=0, **{"global": 0})
