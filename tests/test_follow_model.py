"""The vector-field follower without a GPU: mesh_navigation_amd/csrc/mnav_follow.h compiled for the host (g++
-ffp-contract=off, the flags of the library) -- the stay test, the projection, directionAtPosition, the cost, naiveControl
and the saturations are the device's own source, composed serially in the reference's order over the index the shim of
tests/test_locate_model.py builds -- against tests/follow_model.py, the Python restatement of the reference's lines with the
host libm's acosf.  Every comparison is exact (floats by their bits; any NaN equals any NaN)."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from tests import follow_model as FM
from tests.common import Case
from tests.test_locate_model import CSRC, SHIM as LOCATE_SHIM

SHIM = LOCATE_SHIM + r'''
#include <cstring>
#include "mnav_follow.h"
// n robots through fol_tick; fields: S vector maps of V rows each, one after the other; seed_face may be null
extern "C" void fol_batch(void* h, uint32_t n, const float* pos, const float* dir, const float* up, const uint32_t* face_in, const uint32_t* slot,
                          const uint32_t* seed_face, const float* fields, const float* costs, const double* cfg, uint32_t V, uint32_t F,
                          const float* xyz, const uint32_t* faces, const uint32_t* vf_ptr, const uint32_t* vf, int32_t* code, int32_t* how,
                          uint32_t* face, float* bary, float* pos_out, float* mesh_dir, float* cost, double* cmd)
{
  Host* H = (Host*)h;
  const Index I{ H->nodes.data(), H->pts.data(), H->n_pts, H->n_leaves, loc_root(H->n_leaves) };
  const mnav::WalkMesh Mh{ xyz, faces, vf_ptr, vf, V, F };
  mnav_fol::Config Cf;
  static_assert(sizeof(Cf) == 8 * sizeof(double), "eight doubles");
  std::memcpy(&Cf, cfg, sizeof(Cf));
  VecStack st; st.cap = kStack;
  std::vector<uint32_t> list(mnav::kWalkScratchWords);
  for (uint32_t i = 0; i < n; ++i) {
    const mnav::WalkField Fd = mnav_fol::fol_field(Mh, fields + 3 * (size_t)V * slot[i], seed_face ? seed_face[i] : mnav::kNone);
    const mnav_fol::Result R = mnav_fol::fol_tick(Mh, I, st, Fd, costs, Cf, mnav::w3_load(pos + 3 * (size_t)i), mnav::w3_load(dir + 3 * (size_t)i),
                                                  mnav::w3_load(up + 3 * (size_t)i), face_in[i], list.data());
    code[i] = R.code; how[i] = R.how; face[i] = R.face; cost[i] = R.cost;
    for (int k = 0; k < 3; ++k) bary[3 * (size_t)i + k] = R.bary[k];
    pos_out[3 * (size_t)i] = R.pos.x; pos_out[3 * (size_t)i + 1] = R.pos.y; pos_out[3 * (size_t)i + 2] = R.pos.z;
    mesh_dir[3 * (size_t)i] = R.mesh_dir.x; mesh_dir[3 * (size_t)i + 1] = R.mesh_dir.y; mesh_dir[3 * (size_t)i + 2] = R.mesh_dir.z;
    cmd[2 * (size_t)i] = R.lin; cmd[2 * (size_t)i + 1] = R.ang;
  }
}
extern "C" float fol_acosf(float x) { return mnav::acosf_ref(x); }
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_follow.h"
    d = tmp_path_factory.mktemp("follow_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    vp, u32 = C.c_void_p, C.c_uint32
    L.loc_build.restype = vp
    L.loc_build.argtypes = [u32, vp]
    L.loc_free.argtypes = [vp]
    L.fol_batch.argtypes = [vp, u32] + [vp] * 9 + [u32, u32] + [vp] * 12
    L.fol_acosf.restype = C.c_float
    L.fol_acosf.argtypes = [C.c_float]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Mirror:
    """mnav_follow.h on the host over one mesh"""

    def __init__(self, L, model):
        self.L, self.m = L, model
        self.h = L.loc_build(model.V, _p(model.xyz))
        self.ptr, self.vf = np.ascontiguousarray(model.ptr, np.uint32), np.ascontiguousarray(model.vf, np.uint32)

    def close(self):
        self.L.loc_free(self.h)

    def tick_batch(self, cfg, fields, robots):
        m = self.m
        n = robots["pos"].shape[0]
        fl = np.ascontiguousarray(np.stack(fields), np.float32)
        c = np.array([cfg[k] for k in FM.CFG_NAMES], np.float64)
        r = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in robots.items()}
        out = dict(code=np.zeros(n, np.int32), how=np.zeros(n, np.int32), face=np.zeros(n, np.uint32), bary=np.zeros((n, 3), np.float32),
                   pos=np.zeros((n, 3), np.float32), mesh_dir=np.zeros((n, 3), np.float32), cost=np.zeros(n, np.float32),
                   cmd=np.zeros((n, 2), np.float64))
        self.L.fol_batch(self.h, n, _p(r["pos"]), _p(r["dir"]), _p(r["up"]), _p(r["face_in"]), _p(r["slot"]), _p(r.get("seed_face")), _p(fl),
                         _p(m.costs), _p(c), m.V, m.F, _p(m.xyz), _p(m.faces), _p(self.ptr), _p(self.vf), _p(out["code"]), _p(out["how"]),
                         _p(out["face"]), _p(out["bary"]), _p(out["pos"]), _p(out["mesh_dir"]), _p(out["cost"]), _p(out["cmd"]))
        return out


MESHES = {
    "terrain": lambda: meshgen.terrain(64, 0.1, 6, amplitude=0.6),
    "holes": lambda: meshgen.punched(72, 0.1, 4, drop=0.12),
    "hub": lambda: meshgen.fan_field(spokes=40, rings=6, seed=1),
}
CONFIGS = {
    "default": FM.config(),
    # both saturations bite, a wider cone, a short reach in both search parameters
    "saturating": FM.config(max_lin_velocity=0.8, max_ang_velocity=0.3, ang_vel_factor=4.0, lin_vel_factor=5.0, max_angle=45.0,
                            max_search_radius=0.15, max_search_distance=0.1),
    "slow_wide": FM.config(max_lin_velocity=0.25, max_ang_velocity=1.5, ang_vel_factor=0.5, lin_vel_factor=0.7, max_angle=170.0,
                           max_search_radius=0.7, max_search_distance=1.5),
}


def build_world(name, seed=11):
    """the mesh, its model, three fields (oracle Dijkstra, oracle CVP, synthetic) and their seed faces"""
    mesh = MESHES[name]()
    rng = np.random.default_rng(seed)
    case = Case(mesh, rng.uniform(0.0, 0.8, mesh.V).astype(np.float32), edge_cost_factor=1.0)
    om = case.om
    model = FM.Model(mesh, om, case.costs)
    cen = mesh.xyz[mesh.faces].astype(np.float64).mean(axis=1)
    mid = cen.mean(axis=0)
    order = np.argsort(np.linalg.norm(cen - mid, axis=1))
    goal_face = int(order[0])                                          # a face in the middle of the mesh
    far_face = int(order[int(0.55 * mesh.F)])                         # the robot of the plans: the waves stop a little beyond it
    # Dijkstra: the reference's vector map (dijkstra_mesh_planner.cpp:189-209) over the predecessors of a plan that stops
    # goal_dist_offset beyond the robot vertex: the outer part of the mesh has no vectors
    sv, tv = int(mesh.faces[goal_face][0]), int(mesh.faces[far_face][0])
    dj = om.dijkstra(case.weights, case.costs, sv, tv, goal_dist_offset=0.05)
    f_dij = om.dijkstra_vector_map(dj.pred)
    # CVP: the seed position is a vertex of the seed face (its entry is the zero vector: only the seed rule gives it one)
    goal = mesh.xyz[mesh.faces[goal_face][1]].copy()
    cv = om.cvp(case.weights, case.costs, case.vn, goal, goal_face, far_face, goal_dist_offset=0.05)
    f_cvp = (cv.vecmap * cv.has_vec[:, None]).astype(np.float32)
    # synthetic: towards a point, nothing in a disc around the mesh's middle -- the seed face lies inside the disc
    f_syn = (mid[None, :] - mesh.xyz.astype(np.float64)).astype(np.float32)
    f_syn[np.linalg.norm(mesh.xyz[:, :2] - mid[None, :2], axis=1) < 0.25] = 0
    f_syn[mesh.faces[goal_face]] = 0
    return mesh, model, [f_dij, f_cvp, f_syn], [FM.NONE, goal_face, goal_face], int(order[int(0.4 * mesh.F)])


@pytest.fixture(scope="module", params=list(MESHES))
def world(request, shim):
    mesh, model, fields, seed_faces, start_face = build_world(request.param)
    mirror = Mirror(shim, model)
    mirror.start_face = start_face                                    # a face inside all three fields (the multi-tick leg starts there)
    yield request.param, mesh, model, fields, seed_faces, mirror
    mirror.close()


@pytest.mark.parametrize("cfg_name", list(CONFIGS))
def test_every_family_equals_the_model(world, cfg_name):
    name, mesh, model, fields, seed_faces, mirror = world
    cfg = CONFIGS[cfg_name]
    robots, fam = FM.make_robots(model, len(fields), seed_faces, 300 + list(MESHES).index(name), per_family=60)
    robots = FM.set_angles(model, cfg, fields, robots, fam)
    want = FM.tick_batch(model, cfg, fields, robots)
    got = mirror.tick_batch(cfg, fields, robots)
    FM.assert_same(got, want, (name, cfg_name))
    print(name, cfg_name, "how:", np.bincount(want["how"], minlength=5), "code:", np.bincount(want["code"], minlength=3))
    if cfg_name != "slow_wide":                                       # (its 0.7 m reach finds most "far" faces by the neighbour search)
        ok = FM.assert_every_branch(want, fam, cfg, (name, cfg_name))
        ang_fam = ok & (fam == FM.FAMILIES.index("angles"))
        assert ang_fam.sum() >= 12
    if cfg_name == "saturating":
        ok = want["code"] == FM.OK
        assert (want["cmd"][ok, 0] == cfg["max_lin_velocity"]).any() and (want["cmd"][ok, 1] == cfg["max_ang_velocity"]).any()
        assert (want["cmd"][ok, 0] < cfg["max_lin_velocity"]).any() and (want["cmd"][ok, 1] < cfg["max_ang_velocity"]).any()
    # without the seed faces: the same, except where only the seed rule gives the face a vector
    bare = dict(robots, seed_face=None)
    want0 = FM.tick_batch(model, cfg, fields, bare)
    FM.assert_same(mirror.tick_batch(cfg, fields, bare), want0, (name, cfg_name, "no seed faces"))


def test_sign_phi_zero_and_the_parallel_heading(world):
    name, mesh, model, fields, seed_faces, mirror = world
    cfg = CONFIGS["default"]
    robots, fam = FM.make_robots(model, len(fields), seed_faces, 500, per_family=36)
    robots = FM.set_angles(model, cfg, fields, robots, fam)
    idx = np.nonzero(fam == FM.FAMILIES.index("angles"))[0]
    idx = idx[np.arange(idx.size) % len(FM.ANGLES_DEG) < 2]           # headings = +-mesh_dir
    sub = {k: v[idx] for k, v in robots.items()}
    want = FM.tick_batch(model, cfg, fields, sub)
    FM.assert_same(mirror.tick_batch(cfg, fields, sub), want, (name, "parallel"))
    ok = np.nonzero(want["code"] == FM.OK)[0]
    assert ok.size >= 4
    for j in ok:
        md, d = FM.vec(want["mesh_dir"][j]), FM.vec(sub["dir"][j])
        assert all(c == 0 for c in FM.cross(md, d))                   # sign_phi is +0 (or -0): copysignf(.., -sign_phi)
        # +mesh_dir: phi ~ 0 (or NaN when the dot product rounds above 1: then std::min returns max_ang_velocity);
        # -mesh_dir: phi ~ pi, the angular velocity is -max_ang_velocity * phi / pi or its positive twin
        assert abs(want["cmd"][j, 1]) <= cfg["max_ang_velocity"]


def test_the_seed_rule_gives_the_seed_face_a_vector(world):
    name, mesh, model, fields, seed_faces, mirror = world
    cfg = CONFIGS["default"]
    sf = seed_faces[2]
    rng = np.random.default_rng(5)
    n = 12
    p = FM.face_points(model, np.full(n, sf), rng).astype(np.float32)
    robots = dict(pos=p, dir=np.tile(np.array([1, 0, 0], np.float32), (n, 1)), up=np.tile(np.array([0, 0, 1], np.float32), (n, 1)),
                  face_in=np.full(n, sf, np.uint32), slot=np.full(n, 2, np.uint32), seed_face=np.full(n, sf, np.uint32))
    with_seed = FM.tick_batch(model, cfg, fields, robots)
    without = FM.tick_batch(model, cfg, fields, dict(robots, seed_face=None))
    assert (without["code"] == FM.NO_FIELD).all()                     # three all-zero rows: no vector without the rule
    assert (with_seed["code"] == FM.OK).all() and np.isnan(with_seed["mesh_dir"]).all()   # with it: entries exist, their sum has no direction
    assert (with_seed["cmd"][:, 0] == 0).all() and (with_seed["cmd"][:, 1] == cfg["max_ang_velocity"]).all()   # NaN through :240 and std::min
    FM.assert_same(mirror.tick_batch(cfg, fields, robots), with_seed, (name, "seed"))
    FM.assert_same(mirror.tick_batch(cfg, fields, dict(robots, seed_face=None)), without, (name, "no seed"))


def test_two_hundred_ticks_of_a_unicycle(world):
    name, mesh, model, fields, seed_faces, mirror = world
    cfg = FM.config(max_lin_velocity=0.6, max_angle=60.0, max_ang_velocity=1.0)
    cen = mesh.xyz[mesh.faces].astype(np.float64).mean(axis=1)
    start = mirror.start_face
    hows, n_ok = set(), 0
    for slot in (1, 2):                                               # the CVP field and the synthetic one
        pos = (cen[start] + np.array([0, 0, 0.02])).astype(np.float32)
        d = np.array([0.6, 0.8, 0.0], np.float32)
        up = np.array([0, 0, 1], np.float32)
        face = FM.NONE
        for t in range(200):
            robots = dict(pos=pos[None], dir=d[None], up=up[None], face_in=np.array([face], np.uint32), slot=np.array([slot], np.uint32),
                          seed_face=np.array([seed_faces[slot]], np.uint32))
            want = FM.tick_batch(model, cfg, fields, robots)
            FM.assert_same(mirror.tick_batch(cfg, fields, robots), want, (name, slot, t))
            hows.add(int(want["how"][0]))
            ok = want["code"][0] == FM.OK
            n_ok += int(ok)
            face = int(want["face"][0])                               # NONE after a tick that lost the mesh: the next one searches again
            lin, ang = (want["cmd"][0, 0], want["cmd"][0, 1]) if ok else (0.3, 0.4)   # no command: the robot coasts on a curve
            pos, d = FM.unicycle_step(want["pos"][0], d, up, lin, ang, 0.25)
    assert n_ok >= 100 and hows >= {1, 2, 3}, (n_ok, hows)


def test_the_restated_acosf_is_the_host_libms(shim):
    """the model calls the host libm, the header its restatement: equal on the arguments the controller feeds it"""
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-1, 1, 200000), 1 - 10.0 ** rng.uniform(-9, -1, 50000), -1 + 10.0 ** rng.uniform(-9, -1, 50000),
                        [0.0, -0.0, 1.0, -1.0, 1.0000001, -1.0000001, np.nan, 0.5, -0.5]]).astype(np.float32)
    a = np.array([shim.fol_acosf(float(v)) for v in x], np.float32)
    b = np.array([FM._libm.acosf(float(v)) for v in x], np.float32)
    assert FM.same_bits(a, b)
