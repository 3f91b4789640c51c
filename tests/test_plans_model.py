"""Fleet plans without a GPU (mnav_fleet_plans, mnav_fleet_walk_plans).

mesh_navigation_amd/csrc/mnav_pose.h and mnav_plans.h compiled for the host (g++ with the library's flags: pose_from_position,
plan_pose, walk_pose and the cost loops are the device's own source; classification, scan and id scratch run pass by pass
as the device runs them) against the CPU oracle: the pose function on random and degenerate triples, the whole Dijkstra
call against tests/plans_model.py on the six fields of tests/test_fleet_model.py, the walk poses against
OracleMesh.cvp_poses over rows of OracleMesh.cvp_backtrack.  Everything is compared bit for bit; a NaN matches any NaN."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests import fleet_model as FM
from tests import plans_model as PM
from tests.common import Case
from tests.test_fleet_model import fleet_fields  # noqa: F401  (the fixture with the six fields)
from tests.test_locate_model import CSRC

SHIM = r'''
#include <vector>
#include "mnav_plans.h"
using namespace mnav_fleet;
extern "C" void pose_host(uint32_t n, const float* cur, const float* next, const float* nrm, double* poses, float* lengths, uint32_t* branches)
{
  for (uint32_t i = 0; i < n; ++i) {
    int b = 0;
    lengths[i] = mnav::pose_from_position(mnav::w3_load(cur + 3 * i), mnav::w3_load(next + 3 * i), mnav::w3_load(nrm + 3 * i), poses + 7 * (size_t)i, &b);
    branches[i] = (uint32_t)b;
  }
}
// m plans over V vertices as in the shim of tests/test_fleet_model.py; poses: null, or 7 * off[n] doubles
extern "C" void plans_host(uint32_t n, uint32_t V, uint32_t m, const float* dist, const uint32_t* pred, const uint32_t* seed, const uint32_t* target,
                           const double* offset, const uint8_t* on_device, const uint32_t* plan_code, const uint32_t* slot, const uint32_t* vtx, const float* xyz,
                           const float* vn, const float* start, const float* goal, uint32_t* code, uint32_t* count, float* potential, unsigned long long* off,
                           double* cost, double* poses, uint32_t* counters, uint32_t* branches)
{
  std::vector<Field> fields(m);
  for (uint32_t s = 0; s < m; ++s) {
    Field Fd; Fd.dist = nullptr; Fd.pred = nullptr; Fd.seed = seed[s]; Fd.target = target[s]; Fd.cut = mnav::inf_f(); Fd.code = plan_code[s];
    if (on_device[s]) { Fd.dist = dist + (size_t)V * s; Fd.pred = pred + (size_t)V * s; }
    fleet_cut(Fd, offset[s]);
    fields[s] = Fd;
  }
  fleet_plans_host(n, V, fields.data(), slot, vtx, xyz, vn, start, goal, code, count, potential, off, cost, poses, counters, branches);
}
// one row of m entries, seed first as mnav_fleet_walks packs it: turned into walk order (robot first, k_backtrack's scratch row), then posed
extern "C" double walk_host(uint32_t m, const float* pos, const uint32_t* face, const float* face_normals, uint32_t F, const double* goal_pose, double* poses)
{
  std::vector<float> rp(3 * (size_t)m + 3); std::vector<uint32_t> rf(m + 1);
  for (uint32_t q = 0; q < m; ++q) { for (int k = 0; k < 3; ++k) rp[3 * q + k] = pos[3 * (size_t)(m - 1 - q) + k]; rf[q] = face[m - 1 - q]; }
  WalkRow R; R.pos = rp.data(); R.face = rf.data(); R.m = m;
  for (uint32_t q = 0; q < m; ++q) walk_pose(R, q, face_normals, F, goal_pose, poses + 7 * (size_t)q);
  return walk_cost(R);
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_plans.h"
    d = tmp_path_factory.mktemp("plans_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.pose_host.argtypes = [C.c_uint32] + [C.c_void_p] * 6
    L.plans_host.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 21
    L.walk_host.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.walk_host.restype = C.c_double
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def test_pose_function_equals_the_oracle(shim):
    n = 20000
    rng = np.random.default_rng(7)
    cur, nxt = (rng.uniform(-1, 1, (n + 2, 3)).astype(np.float32) for _ in range(2))
    nrm = np.concatenate([unit_vectors(rng, n), np.array([[0, 0, 1], [0, 0, 1]], np.float32)])
    cur[n], nxt[n] = [0, 0, 0.5], [0, 0, 0]                                   # the direction is parallel to the normal
    nxt[n + 1] = cur[n + 1]                                                  # no direction at all
    poses, lengths, branches = np.zeros((n + 2, 7), np.float64), np.zeros(n + 2, np.float32), np.zeros(n + 2, np.uint32)
    shim.pose_host(n + 2, _p(cur), _p(nxt), _p(nrm), _p(poses), _p(lengths), _p(branches))
    want, want_len = np.zeros((n + 2, 7), np.float64), np.zeros(n + 2, np.float32)
    for i in range(n + 2):
        want[i], want_len[i] = O.pose_from_position(cur[i], nxt[i], nrm[i])
    assert np.array_equal(FM.bits(lengths), FM.bits(want_len))
    assert PM.same_poses(poses, want, "pose function") == 2                 # the two degenerate triples and no other
    taken = np.bincount(branches[:n], minlength=4)
    print("quaternion branches (trace > 0, xx, yy, zz):", list(taken), "told from the result:", PM.quat_branch(want[:n]))
    assert (taken >= 1000).all(), taken                                      # all four branches of getRotation
    for i, length in ((n, 0.5), (n + 1, 0.0)):
        assert np.isnan(poses[i, 3:]).all() and np.array_equal(poses[i, :3], cur[i].astype(np.float64)) and lengths[i] == np.float32(length), i


def mirror(L, W, vn, fields, slots, vtx, start, goal):
    m, n, V = len(fields), len(slots), W.V
    dist, pred = np.full((m, V), np.inf, np.float32), np.tile(np.arange(V, dtype=np.uint32), (m, 1))
    on = np.zeros(m, np.uint8)
    for s, f in enumerate(fields):
        if f.dist is not None:
            dist[s], pred[s], on[s] = f.dist, f.pred, 1
    seed, target = (np.array([getattr(f, k) for f in fields], np.uint32) for k in ("seed", "target"))
    offset = np.array([f.offset for f in fields], np.float64)
    pc = np.array([f.code for f in fields], np.uint32)
    sl, vt = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
    xyz, vn, start, goal = (np.ascontiguousarray(a, np.float32) for a in (W.mesh.xyz, vn, start, goal))
    code, ln, pot, off = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n + 1, np.uint64)
    cost, cnt, br = np.full(n, -1.0, np.float64), np.zeros(4, np.uint32), np.zeros(4, np.uint32)

    def call(poses):
        cnt[:], br[:] = 0, 0
        L.plans_host(n, V, m, _p(dist), _p(pred), _p(seed), _p(target), _p(offset), _p(on), _p(pc), _p(sl), _p(vt), _p(xyz), _p(vn), _p(start), _p(goal), _p(code), _p(ln),
                     _p(pot), _p(off), _p(cost), _p(poses), _p(cnt), _p(br))

    call(None)                                                               # the sizing call: everything but the poses
    sized = (code.copy(), ln.copy(), off.copy(), cost.copy())
    poses = np.full((int(off[n]), 7), -7.0, np.float64)
    call(poses)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(sized, (code, ln, off, cost)))
    return dict(codes=code, path_len=ln, potential=pot, offsets=off, cost=cost, poses=poses, counts=[int(c) for c in cnt], branches=[int(b) for b in br])


def fleet(W, fields, n, zero_rows):
    """n robots over the fields: random vertices, the special ones of tests/test_fleet_model.py; zero_rows: every third
    robot stands on its plan's seed or on no vertex, so rows without poses sit between the others"""
    rng = np.random.default_rng(100 + n)
    slots = rng.integers(0, len(fields), n).astype(np.uint32)
    vtx = rng.integers(0, W.V, n).astype(np.uint32)
    if n > 8:
        vtx[:8] = [fields[int(slots[0])].seed, fields[int(slots[1])].target, W.V, FM.NONE, 0, W.V - 1, fields[int(slots[6])].seed, 1]
    if zero_rows:
        for i in range(0, n, 3):
            vtx[i] = fields[int(slots[i])].seed if (i // 3) % 2 else W.V + 1
    on = np.minimum(vtx, W.V - 1)
    start = (W.mesh.xyz[on] + rng.uniform(-0.03, 0.03, (n, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)).astype(np.float32)
    goal = np.array([W.mesh.xyz[min(f.seed, W.V - 1)] + np.array([0.023, 0.011, 0.004], np.float32) for f in fields], np.float32)
    return slots, vtx, start, goal


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 3 * 256 + 41])
def test_host_mirror_equals_the_model(shim, fleet_fields, n):  # noqa: F811
    W, fields = fleet_fields
    vn = W.om.vertex_normals()
    slots, vtx, start, goal = fleet(W, fields, n, zero_rows=n == 3 * 256 + 41)
    want = PM.run(W.om, vn, fields, W.V, slots, vtx, start, goal)
    got = mirror(shim, W, vn, fields, slots, vtx, start, goal)
    assert PM.same(got, want, n) == 0                                        # no NaN pose among random robots
    assert got["counts"] == want["counts"], (n, got["counts"], want["counts"])
    print(n, "poses", int(want["offsets"][n]), "robots with poses", int((want["path_len"] > 0).sum()), "branches", got["branches"])
    if n >= 257:
        assert all(c > 0 for c in want["counts"]) and int(want["offsets"][n]) > 0
    if n == 3 * 256 + 41:
        ln = want["path_len"]
        between = (ln[1:-1] == 0) & (ln[:-2] > 0) & (ln[2:] > 0)
        assert between.sum() >= 20, between.sum()                            # rows without poses between rows with poses: equal neighbouring offsets


def test_host_mirror_with_random_normals_takes_every_branch(shim, fleet_fields):  # noqa: F811
    """random unit vectors uploaded as "vertex normals": all four branches of getRotation occur inside plans"""
    W, fields = fleet_fields
    vn = unit_vectors(np.random.default_rng(5), W.V)
    n = 257
    slots, vtx, start, goal = fleet(W, fields, n, zero_rows=False)
    want = PM.run(W.om, vn, fields, W.V, slots, vtx, start, goal)
    got = mirror(shim, W, vn, fields, slots, vtx, start, goal)
    assert PM.same(got, want, "random normals") == 0
    print("branches", got["branches"], "told from the oracle's poses", PM.quat_branch(want["poses"]))
    assert all(b > 0 for b in got["branches"]) and all(b > 0 for b in PM.quat_branch(want["poses"])), got["branches"]


def test_host_mirror_with_every_row_empty(shim, fleet_fields):  # noqa: F811
    W, fields = fleet_fields
    n = 300
    slots = (np.arange(n) % 4).astype(np.uint32)
    vtx = np.array([fields[int(s)].seed for s in slots], np.uint32)
    vtx[::3] = W.V + 1
    start, goal = np.zeros((n, 3), np.float32), np.zeros((len(fields), 3), np.float32)
    vn = W.om.vertex_normals()
    want = PM.run(W.om, vn, fields, W.V, slots, vtx, start, goal)
    got = mirror(shim, W, vn, fields, slots, vtx, start, goal)
    assert int(want["offsets"][n]) == 0 and (got["cost"] == 0).all()
    assert PM.same(got, want, "empty") == 0


def test_walk_poses_equal_the_oracle(shim):
    """rows of OracleMesh.cvp_backtrack over an OracleMesh.cvp field: reached walks, a failed walk's partial row (the cap
    of 16 entries is hit) and a row of one entry"""
    case = Case(meshgen.terrain(48, 0.1, 6))
    mesh, om = case.mesh, case.om
    sp = (mesh.xyz[mesh.vertex_at(0.3, 0.35)] + np.array([0.023, 0.011, 0.0], np.float32)).astype(np.float32)
    sf, _ = om.containing_face(sp)
    tp0 = (mesh.xyz[mesh.vertex_at(0.75, 0.8)] + np.array([0.031, 0.017, 0.0], np.float32)).astype(np.float32)
    tf0, _ = om.containing_face(tp0)
    field = om.cvp(case.weights, case.costs, case.vn, sp, int(sf), int(tf0), 1e9)
    assert field.code == 0
    goal_pose = np.array([[sp[0], sp[1], sp[2], 0.1, -0.2, 0.3, 0.9]], np.float64)
    rng = np.random.default_rng(4)
    rows, kinds = [], []
    for v, cap in [(int(x), 4096) for x in rng.integers(0, mesh.V, 12)] + [(mesh.vertex_at(0.8, 0.2), 16), (mesh.vertex_at(0.6, 0.7), 1)]:
        tp = (mesh.xyz[v] + np.array([0.031, 0.017, 0.0], np.float32)).astype(np.float32)
        tf, _ = om.containing_face(tp)
        if not 0 <= tf < mesh.F:
            continue
        rc, ppos, pface = om.cvp_backtrack(field.vecmap, field.has_vec, sp, int(sf), tp, int(tf), step_width=0.1, cap=cap)
        rows.append((ppos, pface))
        kinds.append((rc, len(pface), cap))
    assert sum(1 for rc, m, cap in kinds if rc == 0 and m > 2) >= 5 and (FM.NO_PATH_FOUND, 16, 16) in kinds and (FM.NO_PATH_FOUND, 1, 1) in kinds, kinds
    want = PM.walk_run(om, case.fn, rows, np.zeros(len(rows), np.uint32), goal_pose)
    nan = 0
    for i, (ppos, pface) in enumerate(rows):
        m = len(pface)
        poses = np.full((m, 7), -7.0, np.float64)
        cost = shim.walk_host(m, _p(np.ascontiguousarray(ppos, np.float32)), _p(np.ascontiguousarray(pface, np.uint32)), _p(case.fn), mesh.F, _p(goal_pose), _p(poses))
        lo = int(want["offsets"][i])
        nan += PM.same_poses(poses, want["poses"][lo: lo + m], ("walk", i))
        assert PM.bits64(cost) == PM.bits64(want["cost"][i]), (i, cost, want["cost"][i])
        assert np.array_equal(PM.bits64(poses[m - 1]), PM.bits64(goal_pose[0]))      # the goal pose verbatim
    assert nan == 0
    one = kinds.index((FM.NO_PATH_FOUND, 1, 1))
    assert want["cost"][one] == 0 and want["path_len"][one] == 1
