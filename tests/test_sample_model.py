"""The sampled rollout without a GPU: mesh_navigation_amd/csrc/mnav_sample.h compiled for the host (g++ -ffp-contract=off,
the flags of the library) -- smp_after_tick, smp_score, smp_feasible, smp_better and smp_pick are the device's own source,
smp_run composes the rule with mnav_follow.h's fol_tick serially -- against tests/sample_model.py, the Python restatement of
the specification.  Dijkstra, CVP and synthetic fields with a potential each, the three follower configurations.  Every
comparison is exact (floats and doubles by their bits; any NaN equals any NaN).  Also: the score and pick functions on
hand-made rows, candidate (1, 0, 1, 0) against rol_run (the skipped zero bias), a permuted table, and -- on the model's own
output -- that the fleet reaches every branch of the rule."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests import follow_model as FM
from tests import rollout_model as RM
from tests import sample_model as SM
from tests.common import Case
from tests.test_follow_model import CONFIGS, MESHES, build_world
from tests.test_locate_model import CSRC
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT, FLEET_SEED, SHIM as ROLLOUT_SHIM, Mirror as RolloutMirror, fleet

SHIM = ROLLOUT_SHIM + r'''
#include "mnav_sample.h"

// n robots x K candidates through smp_run from the start, then score and pick; fields / pots: S vector maps / potentials of V
// rows each; par = dt, dist_tolerance, angle_tolerance; smp = w_potential, w_cost, w_time, lethal_cost; every output has n * K
// rows (the picks n); seed_face / goal_pos (with goal_dir) may be null; how: 5 counters
extern "C" void smp_batch(void* h, uint32_t n, uint32_t K, const uint32_t* slot, const uint32_t* seed_face, const float* goal_pos, const float* goal_dir,
                          const float* fields, const float* pots, const float* costs, const double* cfg, const double* par, const double* table, const double* smp,
                          uint32_t ticks, uint32_t V, uint32_t F, const float* xyz, const uint32_t* faces, const uint32_t* vf_ptr, const uint32_t* vf, const float* pos,
                          const float* dir, const float* up, const uint32_t* face, int32_t* status, uint32_t* tk, double* score, float* potential, uint8_t* lethal,
                          double* cost_integral, double* travel, float* pos_out, double* cmd0, float* dir_out, uint32_t* face_out, float* min_goal_dist, uint64_t* how,
                          uint32_t* best_k, double* best_score, double* best_cmd, uint32_t* n_feasible)
{
  Host* H = (Host*)h;
  const Index I{ H->nodes.data(), H->pts.data(), H->n_pts, H->n_leaves, loc_root(H->n_leaves) };
  const mnav::WalkMesh Mh{ xyz, faces, vf_ptr, vf, V, F };
  mnav_fol::Config Cf;
  std::memcpy(&Cf, cfg, sizeof(Cf));
  const mnav_rol::Params P = params(par, goal_pos != nullptr);
  const mnav_smp::Rule Q{ Cf.max_lin_velocity, Cf.max_ang_velocity, (float)smp[3], mnav::GPtr<const uint32_t>(faces), F };
  const mnav_smp::Weights G{ smp[0], smp[1], smp[2], par[0] };
  VecStack st; st.cap = kStack;
  std::vector<uint32_t> list(mnav::kWalkScratchWords);
  const mnav::W3 zero = mnav::w3(0, 0, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const mnav::WalkField Fd = mnav_fol::fol_field(Mh, fields + 3 * (size_t)V * slot[i], seed_face ? seed_face[i] : mnav::kNone);
    for (uint32_t k = 0; k < K; ++k) {
      const size_t r = (size_t)i * K + k;
      mnav_smp::Row W = mnav_smp::smp_start(mnav::w3_load(pos + 3 * (size_t)i), mnav::w3_load(dir + 3 * (size_t)i), mnav::w3_load(up + 3 * (size_t)i), face[i]);
      mnav_smp::smp_run(Mh, I, st, Fd, costs, pots + (size_t)V * slot[i], Cf, P, Q, mnav_smp::smp_cand(mnav::GPtr<const double>(table), k),
                        goal_pos ? mnav::w3_load(goal_pos + 3 * (size_t)i) : zero, goal_dir ? mnav::w3_load(goal_dir + 3 * (size_t)i) : zero, W, ticks, list.data(), how);
      status[r] = W.status; tk[r] = W.ticks; score[r] = mnav_smp::smp_score(W.pot, W.cost_integral, W.ticks, G); potential[r] = W.pot; lethal[r] = (uint8_t)W.lethal;
      cost_integral[r] = W.cost_integral; travel[r] = W.travel; cmd0[2 * r] = W.cmd0[0]; cmd0[2 * r + 1] = W.cmd0[1];
      pos_out[3 * r] = W.pos.x; pos_out[3 * r + 1] = W.pos.y; pos_out[3 * r + 2] = W.pos.z;
      dir_out[3 * r] = W.dir.x; dir_out[3 * r + 1] = W.dir.y; dir_out[3 * r + 2] = W.dir.z;
      face_out[r] = W.face; min_goal_dist[r] = W.min_goal_dist;
    }
  }
  for (uint32_t i = 0; i < n; ++i) {
    const size_t r = (size_t)i * K;
    const mnav_smp::Pick B = mnav_smp::smp_pick(K, status + r, lethal + r, score + r, cmd0 + 2 * r);
    best_k[i] = B.k; best_score[i] = B.score; best_cmd[2 * (size_t)i] = B.cmd[0]; best_cmd[2 * (size_t)i + 1] = B.cmd[1]; n_feasible[i] = B.n_feasible;
  }
}
// smp_score on m hand-made rows; w = w_potential, w_cost, w_time, dt
extern "C" void smp_scores(uint32_t m, const float* pot, const double* cost_integral, const uint32_t* ticks, const double* w, double* score)
{
  const mnav_smp::Weights G{ w[0], w[1], w[2], w[3] };
  for (uint32_t r = 0; r < m; ++r) score[r] = mnav_smp::smp_score(pot[r], cost_integral[r], ticks[r], G);
}
// smp_pick on the K hand-made rows of one robot; out = k, n_feasible; fout = score, cmd[0], cmd[1]
extern "C" void smp_pick_one(uint32_t K, const int32_t* status, const uint8_t* lethal, const double* score, const double* cmd0, uint32_t* out, double* fout)
{
  const mnav_smp::Pick B = mnav_smp::smp_pick(K, status, lethal, score, cmd0);
  out[0] = B.k; out[1] = B.n_feasible; fout[0] = B.score; fout[1] = B.cmd[0]; fout[2] = B.cmd[1];
}
// smp_command: the skipped zero bias and the saturation
extern "C" double smp_command_one(double gain, double bias, double x, double cap) { return mnav_smp::smp_command(gain, bias, x, cap); }
'''


def build_shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_sample.h"
    d = tmp_path_factory.mktemp("sample_shim")
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
    L.smp_batch.argtypes = [vp, u32, u32] + [vp] * 11 + [u32] * 3 + [vp] * 25
    L.smp_scores.argtypes = [u32] + [vp] * 5
    L.smp_pick_one.argtypes = [u32] + [vp] * 6
    L.smp_command_one.restype = C.c_double
    L.smp_command_one.argtypes = [C.c_double] * 4
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Mirror(RolloutMirror):
    """mnav_sample.h (and mnav_rollout.h) on the host over one mesh"""

    def sample(self, cfg, fields, pots, robots, goals, table, dt, ticks, dist_tol=0.0, ang_tol=0.0, sample=None):
        """smp_run for every row, then smp_score and smp_pick: the dict of sample_model.run plus dir, face, min_goal_dist per row"""
        m = self.m
        sample = dict(SM.SAMPLE_DEFAULTS, **(sample or {}))
        table = np.ascontiguousarray(table, np.float64).reshape(-1, 4)
        n, K = robots["pos"].shape[0], table.shape[0]
        fl, pt = np.ascontiguousarray(np.stack(fields), np.float32), np.ascontiguousarray(np.stack(pots), np.float32)
        c = np.array([cfg[k] for k in FM.CFG_NAMES], np.float64)
        par = np.array([dt, dist_tol, ang_tol], np.float64)
        smp = np.array([sample[k] for k in ("w_potential", "w_cost", "w_time", "lethal_cost")], np.float64)
        pos, d, up = (np.ascontiguousarray(robots[k], np.float32) for k in ("pos", "dir", "up"))
        face, slot = np.ascontiguousarray(robots["face_in"], np.uint32), np.ascontiguousarray(robots["slot"], np.uint32)
        sf = None if robots.get("seed_face") is None else np.ascontiguousarray(robots["seed_face"], np.uint32)
        gp = None if goals is None else np.ascontiguousarray(goals[0], np.float32)
        gd = None if goals is None else np.ascontiguousarray(goals[1], np.float32)
        o = dict(status=np.zeros((n, K), np.int32), ticks=np.zeros((n, K), np.uint32), score=np.zeros((n, K), np.float64), potential=np.zeros((n, K), np.float32),
                 lethal=np.zeros((n, K), np.uint8), cost_integral=np.zeros((n, K), np.float64), travel=np.zeros((n, K), np.float64), pos=np.zeros((n, K, 3), np.float32),
                 cmd0=np.zeros((n, K, 2), np.float64), dir=np.zeros((n, K, 3), np.float32), face=np.zeros((n, K), np.uint32), min_goal_dist=np.zeros((n, K), np.float32),
                 how=np.zeros(5, np.uint64), best_k=np.zeros(n, np.uint32), best_score=np.zeros(n, np.float64), best_cmd=np.zeros((n, 2), np.float64),
                 n_feasible=np.zeros(n, np.uint32))
        self.L.smp_batch(self.h, n, K, _p(slot), _p(sf), _p(gp), _p(gd), _p(fl), _p(pt), _p(m.costs), _p(c), _p(par), _p(table), _p(smp), ticks, m.V, m.F, _p(m.xyz),
                         _p(m.faces), _p(self.ptr), _p(self.vf), _p(pos), _p(d), _p(up), _p(face), *[_p(o[k]) for k in o])
        o["how"] = o["how"].astype(np.int64)
        return o


def world_potentials(name, mesh, model):
    """a potential for each of build_world's three fields: the oracle's Dijkstra and CVP distances of the same plans (+inf
    where the wave did not come) and, for the synthetic field, the distance to the point it points to"""
    case = Case(mesh, model.costs, edge_cost_factor=1.0)
    cen = mesh.xyz[mesh.faces].astype(np.float64).mean(axis=1)
    mid = cen.mean(axis=0)
    order = np.argsort(np.linalg.norm(cen - mid, axis=1))
    goal_face, far_face = int(order[0]), int(order[int(0.55 * mesh.F)])
    dj = case.om.dijkstra(case.weights, case.costs, int(mesh.faces[goal_face][0]), int(mesh.faces[far_face][0]), goal_dist_offset=0.05)
    cv = case.om.cvp(case.weights, case.costs, case.vn, mesh.xyz[mesh.faces[goal_face][1]].copy(), goal_face, far_face, goal_dist_offset=0.05)
    syn = np.linalg.norm(mesh.xyz.astype(np.float64) - mid[None, :], axis=1).astype(np.float32)
    return [np.ascontiguousarray(dj.dist, np.float32), np.ascontiguousarray(cv.dist, np.float32), syn]


# follower, an arc to the left, follow but keep left, the arc again (two rows tied in J), half speed keeping right, straight ahead
TABLE = np.array([[1, 0, 1, 0], [0, 0.5, 0, 0.3], [1, 0, 1, 0.2], [0, 0.5, 0, 0.3], [0.5, 0.1, 1, -0.2], [0, 1.0, 0, 0]], np.float64)
TICKS = {"default": 40, "saturating": 40, "slow_wide": 8}     # (slow_wide reaches far and turns fast: after 40 ticks no row is RUNNING)
SAMPLE = dict(w_potential=1.0, w_cost=0.5, w_time=0.1, lethal_cost=0.7)


@pytest.fixture(scope="module", params=list(MESHES))
def world(request, shim):
    mesh, model, fields, seed_faces, start_face = build_world(request.param)
    pots = world_potentials(request.param, mesh, model)
    mirror = Mirror(shim, model)
    robots, goals = fleet(model, len(fields), seed_faces, FLEET_SEED[request.param], per_family=1, drivers=15)
    assert robots["pos"].shape[0] <= 24
    yield request.param, model, fields, pots, robots, goals, mirror
    mirror.close()


@pytest.mark.parametrize("cfg_name", list(CONFIGS))
def test_smp_run_equals_the_model(world, cfg_name):
    name, model, fields, pots, robots, goals, mirror = world
    cfg = CONFIGS[cfg_name]
    want = SM.run(model, cfg, fields, pots, robots, goals, TABLE, DT, TICKS[cfg_name], DIST_TOL, ANG_TOL, SAMPLE)
    got = mirror.sample(cfg, fields, pots, robots, goals, TABLE, DT, TICKS[cfg_name], DIST_TOL, ANG_TOL, SAMPLE)
    print(name, cfg_name, "status:", np.bincount(want["status"].reshape(-1), minlength=4), "lethal:", int(want["lethal"].sum()), "best_k:", want["best_k"],
          "n_feasible:", want["n_feasible"], "how:", want["how"])
    SM.assert_same(got, want, (name, cfg_name), keys=SM.PICKS + SM.ROWS + ("cmd0",))
    assert np.array_equal(got["how"], want["how"])
    # the fleet and the table reach every branch of the rule, by the model alone
    SM.assert_every_branch(want, (name, cfg_name))
    assert want["how"][1] > 0 and want["how"][2] > 0 and want["how"][3] > 0
    # rows 1 and 3 are one candidate: the same bits, and the later one is never picked
    SM.assert_same({k: got[k][:, 3] for k in SM.ROWS}, {k: got[k][:, 1] for k in SM.ROWS}, (name, "candidates 1 and 3"), keys=SM.ROWS)
    assert not (want["best_k"] == 3).any()


def test_without_goals_and_without_seed_faces(world):
    name, model, fields, pots, robots, goals, mirror = world
    cfg = CONFIGS["default"]
    r = dict(robots, seed_face=None)
    want = SM.run(model, cfg, fields, pots, r, None, TABLE, DT, 12, sample=SAMPLE)
    got = mirror.sample(cfg, fields, pots, r, None, TABLE, DT, 12, sample=SAMPLE)
    SM.assert_same(got, want, (name, "no goals"), keys=SM.PICKS + SM.ROWS + ("cmd0",))
    assert RM.REACHED not in set(want["status"].reshape(-1).tolist())


@pytest.mark.parametrize("cfg_name", list(CONFIGS))
def test_the_follower_candidate_is_the_rollout(world, cfg_name):
    """the skipped zero bias: under (1, 0, 1, 0) every state bit of every robot is rol_run's, a -0 command included"""
    name, model, fields, pots, robots, goals, mirror = world
    cfg = CONFIGS[cfg_name]
    got = mirror.sample(cfg, fields, pots, robots, goals, [[1, 0, 1, 0]], DT, 120, DIST_TOL, ANG_TOL, SAMPLE)
    want = mirror.run(cfg, fields, robots, goals, DT, 120, DIST_TOL, ANG_TOL)
    row = {k: got[k][:, 0] for k in ("status", "ticks", "pos", "dir", "face", "travel", "cost_integral", "min_goal_dist")}
    RM.assert_same(row, want, (name, cfg_name), keys=RM.KEYS)
    assert np.array_equal(got["how"], want["how"]) and (want["ticks"] > 8).any()


def test_a_permuted_table_permutes_the_rows(world):
    name, model, fields, pots, robots, goals, mirror = world
    cfg = CONFIGS["default"]
    perm = np.array([4, 2, 5, 0, 3, 1])
    a = mirror.sample(cfg, fields, pots, robots, goals, TABLE, DT, 40, DIST_TOL, ANG_TOL, SAMPLE)
    b = mirror.sample(cfg, fields, pots, robots, goals, TABLE[perm], DT, 40, DIST_TOL, ANG_TOL, SAMPLE)
    SM.assert_same({k: b[k] for k in SM.ROWS + ("cmd0",)}, {k: a[k][:, perm] for k in SM.ROWS + ("cmd0",)}, (name, "permuted"), keys=SM.ROWS + ("cmd0",))
    assert FM.same_bits(b["best_score"], a["best_score"]) and np.array_equal(b["n_feasible"], a["n_feasible"])
    has = a["best_k"] != SM.NONE
    assert np.array_equal(b["best_k"] == SM.NONE, ~has)
    # (best_k and best_cmd may differ: among rows tied in J the pick is the smallest k of the table as given)
    assert FM.same_bits(a["score"][has, a["best_k"][has]], b["score"][has, b["best_k"][has]])
    kb = b["best_k"][has]
    assert FM.same_bits(b["best_cmd"][has], b["cmd0"][has, kb]) and (perm[kb] == a["best_k"][has]).any()


def _pick(shim, status, lethal, score, cmd0=None):
    K = len(score)
    st, le, sc = np.asarray(status, np.int32), np.asarray(lethal, np.uint8), np.asarray(score, np.float64)
    cm = np.arange(1, 2 * K + 1, dtype=np.float64).reshape(K, 2) if cmd0 is None else np.asarray(cmd0, np.float64)
    out, fout = np.zeros(2, np.uint32), np.zeros(3, np.float64)
    shim.smp_pick_one(K, _p(st), _p(le), _p(sc), _p(cm), _p(out), _p(fout))
    model = SM.pick(st, le, sc, cm)
    assert (int(out[0]), int(out[1])) == (model[0], model[3]) and FM.same_bits(fout, np.array([model[1], model[2][0], model[2][1]], np.float64))
    return int(out[0]), int(out[1]), fout.tolist()


def test_score_and_pick_on_hand_made_rows(shim):
    inf, nan = float("inf"), float("nan")
    R, D, O, N = RM.RUNNING, RM.REACHED, RM.OUT_OF_MAP, RM.NO_FIELD
    # equal J: the smaller k; cmd0 of row k is (2 k + 1, 2 k + 2)
    assert _pick(shim, [R, R, R], [0, 0, 0], [2.0, 1.0, 1.0]) == (1, 3, [1.0, 3.0, 4.0])
    assert _pick(shim, [R, D, R, D], [0, 0, 0, 0], [5.0, 5.0, 5.0, 5.0])[:2] == (0, 4)
    # -0 against +0 is a tie: the smaller k, whichever sign it has
    k, _, f = _pick(shim, [R, R], [0, 0], [0.0, -0.0])
    assert k == 0 and np.signbit(f[0]) == False
    k, _, f = _pick(shim, [R, R], [0, 0], [-0.0, 0.0])
    assert k == 0 and np.signbit(f[0]) == True
    # nothing feasible: NONE, +inf, zeros
    assert _pick(shim, [O, N, R, D, R], [0, 0, 1, 1, 0], [1.0, 1.0, 1.0, 1.0, nan]) == (SM.NONE, 0, [inf, 0.0, 0.0])
    # NaN, +inf and -inf are infeasible, whatever stands beside them
    assert _pick(shim, [R, R, R, R], [0, 0, 0, 0], [nan, -inf, inf, 7.0]) == (3, 1, [7.0, 7.0, 8.0])
    # status and the lethal flag decide before J does
    assert _pick(shim, [O, N, R, D, R], [0, 0, 1, 0, 0], [0.0, 0.0, 0.0, 9.0, 8.0]) == (4, 2, [8.0, 9.0, 10.0])
    assert _pick(shim, [D], [0], [-3.5]) == (0, 1, [-3.5, 1.0, 2.0])
    # 130 rows: the minimum far behind the first 64
    sc = np.full(130, 4.0)
    sc[[77, 129]] = 3.0
    assert _pick(shim, np.zeros(130), np.zeros(130), sc)[:2] == (77, 130)
    # the score: double, left to right; an infinite potential makes it infinite, or NaN under a zero weight
    pot, ci, tk = np.array([1.5, inf, inf, nan, 1e30], np.float32), np.array([2.0, 1.0, 1.0, 0.0, -1e300]), np.array([4, 1, 1, 0, 100000], np.uint32)
    for w in ([1.0, 0.5, 0.1, 0.25], [0.0, 1.0, 1.0, 0.1], [1e10, 1e10, 0.0, 0.001]):
        out = np.zeros(5, np.float64)
        shim.smp_scores(5, _p(pot), _p(ci), _p(tk), _p(np.array(w, np.float64)), _p(out))
        want = [SM.score(dict(pot=pot[r], cost_integral=ci[r], ticks=int(tk[r])), dict(w_potential=w[0], w_cost=w[1], w_time=w[2]), w[3]) for r in range(5)]
        assert FM.same_bits(out, np.array(want, np.float64)), (w, out, want)
    assert out[0] == 1e10 * 1.5 + 1e10 * 2.0 and np.isinf(out[1]) and np.isnan(out[3])


def test_a_zero_bias_is_skipped(shim):
    cmd = shim.smp_command_one
    assert np.signbit(cmd(1.0, 0.0, -0.0, 1.0)) and np.signbit(cmd(1.0, -0.0, -0.0, 1.0))      # passed through: -0 stays -0
    assert not np.signbit(cmd(1.0, 1e-300, -0.0, 1.0)) and cmd(1.0, 1e-300, -0.0, 1.0) == 1e-300
    assert cmd(1.0, 0.0, 0.37, 1.0) == 0.37 and cmd(0.0, 0.5, 0.37, 1.0) == 0.5 and cmd(2.0, 0.25, 0.5, 1.0) == 1.0     # the saturation
    assert cmd(1.0, 0.0, float("nan"), 0.8) == 0.8                                                  # std::min caps a NaN command
    for g, b, x, cap in [(1.0, 0.0, -0.0, 1.0), (0.5, -0.2, 0.3, 0.5), (1.0, 0.3, 0.4, 0.5), (-1.0, 0.0, 0.2, 0.5)]:
        assert FM.same_bits(np.float64(cmd(g, b, x, cap)), np.float64(SM.command(g, b, x, cap)))
