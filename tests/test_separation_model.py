"""The fleet rollout without a GPU: mesh_navigation_amd/csrc/mnav_fleet_rollout.h compiled for the host (g++
-ffp-contract=off, the flags of the library) -- the rule (frol_waits, sep_present, sep_d2, sep_meet, sep_close) and the grid
search (sep_range, sep_insert, sep_find, sep_cells, sep_tests, sep_near) are the device's own source, sep_check_host composes
them serially -- against tests/separation_model.py, the O(n^2) numpy restatement of the specification.  Point sets built to break a grid, each
at separation_cell_scale 1.0, the default and 4.0 and at two table sizes; presence under the four flag combinations; the tie
rules; the guard's count; the departure equivalences of include/mnav.h on a mesh; and the fold of a call's check rows into
its statistics (sep_fold) against the model's and on tables written by hand.  Every comparison is exact."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests import follow_model as FM
from tests import rollout_model as RM
from tests import separation_model as SM
from tests.test_follow_model import CONFIGS, build_world
from tests.test_locate_model import CSRC
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT, SHIM as ROLLOUT_SHIM, Mirror, fleet

F32 = np.float32
SCALES = (1.0, 2.0, 4.0)                                              # 2.0: the default (mnav_frol::kDefaultCellScale)

SHIM = ROLLOUT_SHIM + r'''
#include "mnav_fleet_rollout.h"

extern "C" float sep_default_scale() { return mnav_frol::kDefaultCellScale; }
extern "C" uint32_t sep_table_size(uint32_t n) { return mnav_frol::sep_table_size(n); }
// the cells a robot at x searches on one axis, and the cell of x itself
extern "C" void sep_axis_cells(float r, float scale, float x, int* out)
{
  const mnav_frol::Grid G = mnav_frol::sep_grid(r, scale);
  mnav_frol::sep_axis(G, x, &out[0], &out[1]);
  out[2] = mnav_frol::sep_cell(x, G.h);
}
// one check over n robots; rows: the seven per-robot arrays; chk: kCheckWords.  Returns 1 when the pair pass ran
extern "C" int sep_check(uint32_t n, const float* pos, const int32_t* status, const uint32_t* start_tick, uint32_t tick, uint32_t flags, float r, float scale,
                         uint32_t table_size, uint64_t max_tests, uint32_t* near_checks, uint32_t* max_partners, uint32_t* first_near_tick,
                         uint32_t* first_near_robot, float* min_sep2, uint32_t* min_sep_tick, uint32_t* min_sep_robot, uint64_t* chk)
{
  const mnav_frol::Rows A{ near_checks, max_partners, first_near_tick, first_near_robot, min_sep2, min_sep_tick, min_sep_robot };
  return mnav_frol::sep_check_host(n, pos, status, start_tick, tick, flags, mnav_frol::sep_grid(r, scale), table_size, max_tests, A, chk) ? 1 : 0;
}
// The fleet rollout serially: per call tick every robot that does not wait (frol_waits) has one tick of rol_run, then the
// trace row, then the check.  Arguments as rol_batch, then start_tick (null: all 0), the separation (r <= 0: none) and the
// rows; chk: kCheckWords per check
extern "C" void frol_batch(void* h, uint32_t n, const uint32_t* slot, const uint32_t* seed_face, const float* goal_pos, const float* goal_dir, const float* fields,
                           const float* costs, const double* cfg, const double* par, uint32_t ticks, uint32_t stride, uint32_t V, uint32_t F, const float* xyz,
                           const uint32_t* faces, const uint32_t* vf_ptr, const uint32_t* vf, int32_t* status, uint32_t* tk, float* pos, float* dir,
                           const float* up, uint32_t* face, double* travel, double* cost_integral, float* min_goal_dist, float* trace, uint64_t* how,
                           const uint32_t* start_tick, float r, float scale, uint32_t check_stride, uint32_t flags, uint64_t max_tests, uint32_t* near_checks,
                           uint32_t* max_partners, uint32_t* first_near_tick, uint32_t* first_near_robot, float* min_sep2, uint32_t* min_sep_tick,
                           uint32_t* min_sep_robot, uint64_t* chk)
{
  Host* H = (Host*)h;
  const Index I{ H->nodes.data(), H->pts.data(), H->n_pts, H->n_leaves, loc_root(H->n_leaves) };
  const mnav::WalkMesh Mh{ xyz, faces, vf_ptr, vf, V, F };
  mnav_fol::Config Cf;
  std::memcpy(&Cf, cfg, sizeof(Cf));
  const mnav_rol::Params P = params(par, goal_pos != nullptr);
  const ::Rows A{ status, tk, pos, dir, up, face, travel, cost_integral, min_goal_dist };
  const mnav_frol::Rows S{ near_checks, max_partners, first_near_tick, first_near_robot, min_sep2, min_sep_tick, min_sep_robot };
  VecStack st; st.cap = kStack;
  std::vector<uint32_t> list(mnav::kWalkScratchWords);
  const uint32_t rows = stride ? ticks / stride : 0;
  const mnav::W3 zero = mnav::w3(0, 0, 0);
  for (uint32_t t = 1; t <= ticks; ++t) {
    for (uint32_t i = 0; i < n; ++i) {
      if (!(start_tick && mnav_frol::frol_waits(t, start_tick[i]))) {
        const mnav::WalkField Fd = mnav_fol::fol_field(Mh, fields + 3 * (size_t)V * slot[i], seed_face ? seed_face[i] : mnav::kNone);
        State R = load(A, i);
        mnav_rol::rol_run(Mh, I, st, Fd, costs, Cf, P, goal_pos ? mnav::w3_load(goal_pos + 3 * (size_t)i) : zero, goal_dir ? mnav::w3_load(goal_dir + 3 * (size_t)i) : zero,
                          R, 1, 0, nullptr, list.data(), how);
        store(A, i, R);
      }
      if (stride && t % stride == 0) std::memcpy(trace + 3 * ((size_t)rows * i + t / stride - 1), pos + 3 * (size_t)i, 12);
    }
    if (r > 0.f && t % check_stride == 0)
      mnav_frol::sep_check_host(n, pos, status, start_tick, t, flags, mnav_frol::sep_grid(r, scale), mnav_frol::sep_table_size(n), max_tests, S,
                                chk + (size_t)mnav_frol::kCheckWords * (t / check_stride - 1));
  }
}
// sep_fold over the rows of `checks` checks and three of the robots' columns; out: checks_run, checks_skipped,
// first_skipped_tick, robots_near, near_pairs, max_pairs, max_pairs_tick, min_pair (2), tests, max_cell; *min_out: min_sep2
extern "C" void sep_fold_stats(const uint64_t* chk, uint32_t checks, uint32_t check_stride, uint32_t n, const uint32_t* near_checks, const float* min_sep2,
                               const uint32_t* min_sep_robot, uint64_t* out, float* min_out)
{
  mnav_frol::SepStats S;
  mnav_frol::sep_fold(chk, checks, check_stride, n, near_checks, min_sep2, min_sep_robot, S);
  out[0] = S.checks_run; out[1] = S.checks_skipped; out[2] = S.first_skipped_tick; out[3] = S.robots_near; out[4] = S.near_pairs; out[5] = S.max_pairs;
  out[6] = S.max_pairs_tick; out[7] = S.min_pair[0]; out[8] = S.min_pair[1]; out[9] = S.tests; out[10] = S.max_cell;
  *min_out = S.min_sep2;
}
'''


def build_shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_fleet_rollout.h"
    d = tmp_path_factory.mktemp("separation_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    L.loc_build.restype = vp
    L.loc_build.argtypes = [u32, vp]
    L.loc_free.argtypes = [vp]
    L.rol_batch.argtypes = [vp, u32] + [vp] * 8 + [u32] * 4 + [vp] * 15
    L.sep_default_scale.restype = f32
    L.sep_table_size.restype = u32
    L.sep_table_size.argtypes = [u32]
    L.sep_axis_cells.argtypes = [f32, f32, f32, vp]
    L.sep_check.restype = C.c_int
    L.sep_check.argtypes = [u32, vp, vp, vp, u32, u32, f32, f32, u32, C.c_uint64] + [vp] * 8
    L.frol_batch.argtypes = [vp, u32] + [vp] * 8 + [u32] * 4 + [vp] * 15 + [vp, f32, f32, u32, u32, C.c_uint64] + [vp] * 8
    L.sep_fold_stats.argtypes = [vp, u32, u32, u32] + [vp] * 5
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_check(L, pos, radius, scale, rows=None, status=None, start_tick=None, tick=1, flags=0, table_size=None, max_tests=2 ** 63):
    """sep_check_host on one point set; returns the rows (folded into `rows` when given), the check's row and whether it ran"""
    pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    n = pos.shape[0]
    rows = SM.start_rows(n) if rows is None else rows
    status = np.zeros(n, np.int32) if status is None else np.ascontiguousarray(status, np.int32)
    st = None if start_tick is None else np.ascontiguousarray(start_tick, np.uint32)
    chk = np.zeros(4, np.uint64)
    ran = L.sep_check(n, _p(pos), _p(status), _p(st), tick, flags, radius, scale, table_size or L.sep_table_size(n), max_tests,
                      *[_p(rows[k]) for k in SM.SEP_KEYS], _p(chk))
    return rows, dict(tests=int(chk[0]), ordered=int(chk[1]), max_cell=int(chk[2]), skipped=int(chk[3])), bool(ran)


def brute(pos, radius, status=None, waiting=None, flags=0, tick=1, rows=None):
    pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    n = pos.shape[0]
    rows = SM.start_rows(n) if rows is None else rows
    status = np.zeros(n, np.int32) if status is None else np.asarray(status, np.int32)
    waiting = np.zeros(n, bool) if waiting is None else waiting
    near = SM.check(rows, pos, SM.present(status, waiting, flags, pos), radius, tick)
    return rows, near


def against_brute(L, pos, radius, what, small_table=False):
    """the point set at every scale (and, when asked, in the smallest table that holds it) against the brute force"""
    pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    n = pos.shape[0]
    want, near = brute(pos, radius)
    n_present = int(np.isfinite(pos).all(axis=1).sum())
    tables = [None] + ([1 << int(n).bit_length()] if small_table else [])
    for scale in SCALES:
        for table in tables:
            got, chk, ran = host_check(L, pos, radius, scale, table_size=table)
            SM.assert_same_rows(got, want, (what, scale, table))
            assert ran and chk["ordered"] == int(near.sum()) and chk["tests"] >= chk["ordered"] + n_present, (what, scale, chk)
    return want, near


def up(x, k=1):
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(np.inf))
    return x


def down(x, k=1):
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(-np.inf))
    return x


def test_the_default_scale_is_one_of_the_scales_tested(shim):
    assert shim.sep_default_scale() in SCALES and 1.0 in SCALES and 4.0 in SCALES


def test_exactly_at_the_radius_and_one_float_beyond(shim):
    r = 0.5
    pts = np.array([[1, 0, 0], [1.5, 0, 0],                           # d2 == r2 exactly
                    [0, 40, 0], [up(0.5), 40, 0],                     # the coordinate one float beyond: d2 > r2
                    [0, 0, 80], [0, 0, 80 + 0.5], [0, 0, 80 - 0.5],   # ... on another axis, both sides
                    [-7, -7, -7], [-7 - 0.5, -7, -7], [down(-7.5), -7, -7 + 0.0]], F32)
    want, near = against_brute(shim, pts, r, "at the radius")
    d2 = SM.d2_matrix(pts)
    assert d2[0, 1] == F32(0.25) and near[0, 1] and d2[2, 3] > F32(0.25) and not near[2, 3]
    assert near[4, 5] and near[4, 6] and not near[5, 6] and near[7, 8] and not near[7, 9]
    assert want["min_sep2"][0] == F32(0.25) and want["first_near_robot"][2] == SM.NONE and want["max_partners"][4] == 2
    # a 3-4-5 triangle scaled so that every square is exact
    pts = np.array([[0, 0, 0], [0.375, 0.5, 0], [0, 1000, 0], [0.375, 1000.5, up(0)]], F32)
    want, near = against_brute(shim, pts, 0.625, "3-4-5")
    assert SM.d2_matrix(pts)[0, 1] == F32(0.625) * F32(0.625) and near[0, 1]


@pytest.mark.parametrize("radius", [0.5, 0.1, 0.3])
def test_pairs_that_straddle_cell_boundaries(shim, radius):
    r = F32(radius)
    pts = []
    for scale in SCALES:
        h = F32(F32(scale) * r)
        for axis in range(3):
            for k in (-3, -1, 0, 1, 2):
                for g, (a, b) in enumerate([(-0.3, 0.3), (-0.05, 0.9), (-0.999, 0.0), (-0.6, 0.6), (0.0, 0.0)]):
                    base = np.zeros(3)
                    base[(axis + 1) % 3] = 50.0 * (len(pts) // 2 + 1) * radius       # every group far from every other
                    for off in (a, b):
                        p = base.copy()
                        p[axis] = float(k) * float(h) + off * radius
                        pts.append(p)
    pts = np.array(pts, F32)
    want, near = against_brute(shim, pts, radius, "straddling")
    assert near.any() and (want["near_checks"] == 0).any() and near.sum() >= len(pts) // 2


def test_a_quotient_that_rounds_up_to_an_integer(shim):
    """x < k h as real numbers but fl(x / h) == k: the robot counts as standing in cell k although it stands in k - 1, which
    is where floorf(x / h) of two coordinates a radius apart can come to differ by 2 at scale 1.  Each such x with the
    farthest partner below it and the farthest above it that are still near."""
    found, spread = 0, set()
    for radius in (0.1, 0.3, 0.7, 1e-3):
        h = F32(radius)                                              # scale 1
        r2 = h * h
        pts = []
        for k in [k for a in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 100, 129, 1000, 1025) for k in (a, -a)]:
            for x in (down(F32(k) * h), F32(k) * h, down(F32(k) * h, 2), up(F32(k) * h)):
                if not (float(x) < k * float(h) and np.floor(x / h) == k):
                    continue
                lo, hi = down(F32(x - h), 3), up(F32(x + h), 3)
                while (x - lo) * (x - lo) > r2:
                    lo = up(lo)
                while (x - hi) * (x - hi) > r2:
                    hi = down(hi)
                y = 30.0 * radius * (len(pts) // 3 + 1)
                pts += [[x, y, 0], [lo, y, 0], [hi, y, 0]]
                spread.add(int(np.floor(x / h) - np.floor(lo / h)))
                break
        assert len(pts) >= 6, radius
        found += len(pts) // 3
        P = np.array(pts, F32)
        want, near = against_brute(shim, P, radius, ("rounds up", radius))
        assert near[0::3, 1::3].diagonal().all() and near[0::3, 2::3].diagonal().all() and not near[1::3, 2::3].diagonal().any()
        assert (want["max_partners"][0::3] == 2).all()
    print("pairs:", found, "floor differences met:", sorted(spread))
    assert found >= 16


def test_the_search_range_holds_every_near_coordinate(shim):
    """the proof obligation on one axis, sampled: whenever fl(fl(a - b)^2) <= r2 the cell of b lies in the range of a"""
    rng = np.random.default_rng(3)
    out = np.zeros(3, np.int32)
    for radius in (0.1, 0.25, 1.0, 3e-5, 1e4, 4e-20, 3e-23):
        r = F32(radius)
        r2 = r * r
        for scale in (1.0, 1.5, 2.0, 4.0):
            for centre in (0.0, 1.0, -3.0, 1e3, -1e6, 5e8, 1e30):
                for _ in range(60):
                    a = F32(centre + rng.uniform(-6, 6) * radius)
                    for b in (F32(a - r), F32(a + r), up(F32(a - r)), down(F32(a + r)), down(F32(a - r)), up(F32(a + r)), F32(a + rng.uniform(-1, 1) * radius)):
                        with np.errstate(over="ignore"):
                            d = F32(a - b)
                            if not d * d <= r2:
                                continue
                        shim.sep_axis_cells(r, scale, a, _p(out))
                        lo, hi = int(out[0]), int(out[1])
                        shim.sep_axis_cells(r, scale, b, _p(out))
                        assert lo <= int(out[2]) <= hi and hi - lo <= (5 if radius > 1e-17 else 7), (radius, scale, a, b, lo, hi, out)


def test_coincident_robots_a_lone_robot_and_non_finite_coordinates(shim):
    r = 0.4
    pts = np.array([[2, 3, 4]] * 5 + [[2.1, 3, 4], [9, 9, 9]], F32)
    want, near = against_brute(shim, pts, r, "coincident")
    assert (want["min_sep2"][:5] == 0).all() and want["first_near_robot"].tolist()[:6] == [1, 0, 0, 0, 0, 0] and want["max_partners"][0] == 5
    assert want["near_checks"][6] == 0 and want["min_sep2"][6] == np.inf and want["min_sep_robot"][6] == SM.NONE
    one, _ = against_brute(shim, np.array([[1, 2, 3]], F32), r, "n = 1")
    assert one["near_checks"][0] == 0
    # a robot with a NaN or an infinite coordinate is not present: it has no partner and is nobody's
    pts = np.array([[0, 0, 0], [0.1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0.05, 0, -np.inf], [0.2, 0, 0]], F32)
    want, near = against_brute(shim, pts, r, "non-finite")
    assert want["near_checks"].tolist() == [1, 1, 0, 0, 0, 1] and not near[2:5].any() and not near[:, 2:5].any() and want["max_partners"][0] == 2


def test_seventy_robots_in_one_cell(shim):
    rng = np.random.default_rng(5)
    r = 0.5
    pts = (np.array([10.2, -3.3, 0.7]) + rng.uniform(0, 0.25, (70, 3))).astype(F32)
    want, near = against_brute(shim, pts, r, "70 in a cell")
    assert (want["max_partners"] == 69).all() and near.sum() == 70 * 69
    for scale in SCALES:
        _, chk, _ = host_check(shim, pts, r, scale)
        assert chk["max_cell"] == 70 and chk["tests"] == 70 * 70


def test_many_cells_collisions_and_wrap_around(shim):
    """4 000 robots in about as many cells, in a table of 4 096 slots: probe sequences run into each other and round the end"""
    rng = np.random.default_rng(6)
    r = 0.35
    grid = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3) - np.array([10, 10, 5])
    pts = (grid * 0.9 + rng.uniform(-0.4, 0.4, grid.shape)).astype(F32)
    assert pts.shape[0] == 4000
    want, near = against_brute(shim, pts, r, "many cells", small_table=True)
    assert near.any() and (want["near_checks"] == 0).sum() > 1000 and (want["max_partners"] >= 2).any()


def test_coordinates_near_a_million_and_beyond_the_grid(shim):
    r = 0.1
    x = np.float32(1e6)
    line = np.array([[x + 0.0625 * k, -x, 0.5 * x] for k in (0, 1, 3, 6, 7, 8)], F32)       # ulp(1e6) = 0.0625: 0.0625 is near, 0.125 is not
    want, near = against_brute(shim, line, r, "1e6")
    assert near[0, 1] and not near[1, 2] and near[3, 4] and near[4, 5] and not near[3, 5] and want["max_partners"][4] == 2
    # x / h beyond 2^20: the cell coordinates saturate, pairs are still found and far robots still told apart
    far = np.array([[1e9, 0, 0], [1e9, 0, 0], [1e9 + 64, 0, 0], [-3e38, 3e38, 0], [3e38, 3e38, 0], [3e38, 3e38, 0], [-1e12, -1e12, -1e12]], F32)
    want, near = against_brute(shim, far, r, "saturated")
    assert near[0, 1] and not near[0, 2] and near[4, 5] and not near[3, 4] and want["near_checks"][6] == 0
    # a radius so small that r2 is subnormal, and one so large that r2 nearly overflows
    tiny = np.array([[0, 0, 0], [1e-23, 0, 0], [5e-23, 0, 0], [0, 1e-20, 0]], F32)
    want, near = against_brute(shim, tiny, 3e-23, "tiny radius")
    assert near[0, 1] and not near[0, 2] and F32(3e-23) * F32(3e-23) < np.finfo(F32).tiny
    big = np.array([[0, 0, 0], [1e19, 0, 0], [-1e19, 1e18, 0], [3e19, 0, 0]], F32)
    want, near = against_brute(shim, big, 1.5e19, "huge radius")
    assert near[0, 1] and near[0, 2] and not near[0, 3] and not near[1, 2]


def test_presence_under_the_four_flag_combinations(shim):
    # 0 running, 1 waiting, 2 reached, 3 out of the map, 4 no field, 5 running far away; all but 5 within the radius of each other
    pts = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0.1, 0.1, 0], [9, 9, 9]], F32)
    status = np.array([RM.RUNNING, RM.RUNNING, RM.REACHED, RM.OUT_OF_MAP, RM.NO_FIELD, RM.RUNNING], np.int32)
    start = np.array([0, 7, 0, 0, 0, 0], np.uint32)
    seen = {}
    for flags in (0, SM.WAITING_PRESENT, SM.REACHED_PRESENT, SM.WAITING_PRESENT | SM.REACHED_PRESENT):
        for tick in (7, 8):                                           # robot 1 waits at tick 7 and has departed at tick 8
            want, near = brute(pts, 0.3, status, tick <= start.astype(np.int64), flags, tick)
            for scale in SCALES:
                got, chk, _ = host_check(shim, pts, 0.3, scale, status=status, start_tick=start, tick=tick, flags=flags)
                SM.assert_same_rows(got, want, (flags, tick, scale))
            seen[(flags, tick)] = int(want["max_partners"][0])
    # robot 0 sees the two stranded robots always, the waiting and the reached one only under their flags
    assert seen == {(0, 7): 2, (0, 8): 3, (1, 7): 3, (1, 8): 3, (2, 7): 3, (2, 8): 4, (3, 7): 4, (3, 8): 4}


def test_the_tie_rules_and_the_first_check_that_attains_the_minimum(shim):
    r = 1.0
    # robot 0 between 1 and 2 at the same distance (ties to the smaller index), 3 closer later
    checks = [np.array([[0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [5, 0, 0]], F32),
              np.array([[0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0, 0.25, 0]], F32),
              np.array([[0, 0, 0], [0.5, 0, 0], [0, -0.25, 0], [0, 0.25, 0]], F32),      # 2 and 3 tie at the minimum reached before: neither tick nor robot change
              np.array([[0, 0, 0], [9, 0, 0], [9, 9, 0], [0, 9, 0]], F32)]
    for scale in SCALES:
        got, want = SM.start_rows(4), SM.start_rows(4)
        for t, pts in enumerate(checks):
            brute(pts, r, tick=3 * (t + 1), rows=want)
            host_check(shim, pts, r, scale, rows=got, tick=3 * (t + 1))
        SM.assert_same_rows(got, want, scale)
    assert (want["first_near_tick"][0], want["first_near_robot"][0]) == (3, 1) and (want["min_sep_tick"][0], want["min_sep_robot"][0]) == (6, 3)
    assert want["near_checks"][0] == 3 and want["max_partners"][0] == 3 and want["min_sep2"][0] == F32(0.0625)
    assert want["first_near_robot"][0] != want["min_sep_robot"][0] and (want["first_near_tick"][3], want["first_near_robot"][3]) == (6, 0)


def test_the_guard_counts_the_tests_and_skips_above_the_bound(shim):
    n, r = 200, 0.25
    stack = np.tile(np.array([[1, 2, 3]], F32), (n, 1))
    for scale in SCALES:
        rows, chk, ran = host_check(shim, stack, r, scale, max_tests=1000)
        assert not ran and chk == dict(tests=n * n, ordered=0, max_cell=n, skipped=1)
        SM.assert_same_rows(rows, SM.start_rows(n), "skipped")       # the "never" values
        rows, chk, ran = host_check(shim, stack, r, scale, max_tests=n * n)          # T == the bound: served
        assert ran and chk["ordered"] == n * (n - 1)
        SM.assert_same_rows(rows, brute(stack, r)[0], "served")
    # robots at least 8 r apart: with cells of at most 2 r a robot examines no cell but its own, T is exactly n
    apart = (np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3) * 8 * r - 5.0).astype(F32)
    for scale in (1.0, 2.0):
        rows, chk, ran = host_check(shim, apart, r, scale, max_tests=apart.shape[0])
        assert ran and chk["tests"] == apart.shape[0] and chk["ordered"] == 0 and chk["max_cell"] == 1


# -- departures and the whole call, on a mesh ------------------------------------------------------------------------

TICKS, RADIUS = 60, 0.35
START = np.array([0, 1, 7, 59, 60, 61, 300, 0, 3, 0, 20, 0, 0, 2, 0, 0, 0, 5, 0, 0, 0, 0, 0, 1, 0, 4])


def with_stranded(model, robots, goals, k=2, gap=0.1):
    """the fleet plus k robots beside the mesh, `gap` apart: out of the map at their first tick, obstacles to each other"""
    hi = np.nanmax(model.xyz.astype(np.float64), axis=0)
    pos = np.array([[hi[0] + 3.0 + gap * j, hi[1] + 3.0, hi[2]] for j in range(k)], F32)
    extra = dict(pos=pos, dir=np.tile(np.array([1, 0, 0], F32), (k, 1)), up=np.tile(np.array([0, 0, 1], F32), (k, 1)), face_in=np.full(k, FM.NONE, np.uint32),
                 slot=np.zeros(k, np.uint32), seed_face=None if robots.get("seed_face") is None else np.asarray(robots["seed_face"])[:k])
    out = {key: (None if robots[key] is None else np.concatenate([robots[key], extra[key]])) for key in robots}
    return out, (np.concatenate([goals[0], goals[0][:k]]), np.concatenate([goals[1], goals[1][:k]]))


class FleetMirror(Mirror):
    def run_fleet(self, cfg, fields, robots, goals, ticks, start_tick=None, trace_stride=1, radius=0.0, scale=2.0, check_stride=1, flags=0, max_tests=2 ** 63):
        m = self.m
        n = robots["pos"].shape[0]
        S = dict(status=np.zeros(n, np.int32), ticks=np.zeros(n, np.uint32), pos=np.array(robots["pos"], F32), dir=np.array(robots["dir"], F32),
                 face=np.array(robots["face_in"], np.uint32), travel=np.zeros(n), cost_integral=np.zeros(n), min_goal_dist=np.full(n, np.inf, F32))
        fl = np.ascontiguousarray(np.stack(fields), F32)
        c = np.array([cfg[k] for k in FM.CFG_NAMES], np.float64)
        par = np.array([DT, DIST_TOL, ANG_TOL], np.float64)
        upv, slot = np.ascontiguousarray(robots["up"], F32), np.ascontiguousarray(robots["slot"], np.uint32)
        sf = None if robots.get("seed_face") is None else np.ascontiguousarray(robots["seed_face"], np.uint32)
        gp, gd = (None, None) if goals is None else (np.ascontiguousarray(goals[0], F32), np.ascontiguousarray(goals[1], F32))
        trace = np.zeros((n, ticks // trace_stride, 3), F32) if trace_stride else None
        how = np.zeros(5, np.uint64)
        st = None if start_tick is None else np.ascontiguousarray(start_tick, np.uint32)
        rows = SM.start_rows(n)
        chk = np.zeros((max(ticks // check_stride, 1), 4), np.uint64)
        self.L.frol_batch(self.h, n, _p(slot), _p(sf), _p(gp), _p(gd), _p(fl), _p(m.costs), _p(c), _p(par), ticks, trace_stride, m.V, m.F, _p(m.xyz),
                          _p(m.faces), _p(self.ptr), _p(self.vf), _p(S["status"]), _p(S["ticks"]), _p(S["pos"]), _p(S["dir"]), _p(upv), _p(S["face"]),
                          _p(S["travel"]), _p(S["cost_integral"]), _p(S["min_goal_dist"]), _p(trace), _p(how), _p(st), radius, scale, check_stride, flags,
                          max_tests, *[_p(rows[k]) for k in SM.SEP_KEYS], _p(chk))
        return dict(S, trace=trace, how=how.astype(np.int64), **rows, chk=chk)


@pytest.fixture(scope="module")
def built():
    return build_world("terrain")


@pytest.fixture(scope="module")
def world(shim, built):
    mesh, model, fields, seed_faces, start_face = built
    mirror = FleetMirror(shim, model)
    robots, goals = with_stranded(model, *fleet(model, len(fields), seed_faces, 40, per_family=1, drivers=15))
    assert robots["pos"].shape[0] == START.shape[0]
    cfg = CONFIGS["default"]
    whole = SM.departures(model, cfg, fields, robots, goals, DT, TICKS, DIST_TOL, ANG_TOL)
    late = SM.departures(model, cfg, fields, robots, goals, DT, TICKS, DIST_TOL, ANG_TOL, START)
    yield model, fields, robots, goals, mirror, cfg, whole, late
    mirror.close()


def test_without_start_ticks_the_call_is_the_rollout(world):
    model, fields, robots, goals, mirror, cfg, whole, late = world
    rollout = mirror.run(cfg, fields, robots, goals, DT, TICKS, DIST_TOL, ANG_TOL, trace_stride=1)
    got = mirror.run_fleet(cfg, fields, robots, goals, TICKS)
    RM.assert_same(got, rollout, "no start ticks")
    RM.assert_same(got, whole, "the model")
    assert np.array_equal(got["how"], rollout["how"])
    zeros = mirror.run_fleet(cfg, fields, robots, goals, TICKS, start_tick=np.zeros_like(START))
    RM.assert_same(zeros, rollout, "start ticks of 0")


def test_departures_shorten_the_run_and_shift_the_trace(world):
    model, fields, robots, goals, mirror, cfg, whole, late = world
    n = START.shape[0]
    got = mirror.run_fleet(cfg, fields, robots, goals, TICKS, start_tick=START)
    RM.assert_same(got, late, "start ticks")
    assert np.array_equal(got["how"], late["how"])
    rollout = mirror.run(cfg, fields, robots, goals, DT, TICKS, DIST_TOL, ANG_TOL, trace_stride=1)
    for i in range(n):
        s = min(int(START[i]), TICKS)
        # the rows of the first s ticks repeat the start position, the others are the rollout's first TICKS - s rows
        assert FM.same_bits(got["trace"][i, :s], np.repeat(robots["pos"][i][None, :], s, axis=0)), i
        assert FM.same_bits(got["trace"][i, s:], rollout["trace"][i, : TICKS - s]), i
        short = mirror.run(cfg, fields, {k: (None if v is None else v[i:i + 1]) for k, v in robots.items()}, (goals[0][i:i + 1], goals[1][i:i + 1]), DT,
                           max(TICKS - s, 1), DIST_TOL, ANG_TOL) if s < TICKS else None
        if short is not None:
            RM.assert_same({k: got[k][i:i + 1] for k in RM.KEYS}, short, ("per robot", i), keys=RM.KEYS)
    # a robot whose start tick is at or beyond the call's ticks comes back as it went in
    for i in np.nonzero(START >= TICKS)[0]:
        assert got["status"][i] == RM.RUNNING and got["ticks"][i] == 0 and got["face"][i] == robots["face_in"][i] and got["travel"][i] == 0
        assert FM.same_bits(got["pos"][i], robots["pos"][i]) and FM.same_bits(got["dir"][i], robots["dir"][i]) and np.isinf(got["min_goal_dist"][i])
    # the trace at stride 7 is the stride-1 trace thinned out
    t7 = mirror.run_fleet(cfg, fields, robots, goals, TICKS, start_tick=START, trace_stride=7)
    assert FM.same_bits(t7["trace"], SM.thin(late["trace"], 7))
    # resuming: 25 + 35 ticks with the start ticks reduced by the ticks already run
    assert (late["status"] != RM.RUNNING).any() and (late["ticks"] == TICKS).any()


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("check_stride", [1, 7])
def test_the_whole_call_equals_the_model(world, flags, check_stride):
    model, fields, robots, goals, mirror, cfg, whole, late = world
    want = SM.separation(late["trace"], late["status_at"], START, RADIUS, check_stride, flags)
    outs = [mirror.run_fleet(cfg, fields, robots, goals, TICKS, start_tick=START, radius=RADIUS, scale=s, check_stride=check_stride, flags=flags) for s in SCALES]
    for got in outs:
        SM.assert_same_rows(got, want, (flags, check_stride))
        RM.assert_same(got, late, "state")
        served = got["chk"][: TICKS // check_stride]
        assert np.array_equal(served[:, 1].astype(np.int64), 2 * want["pairs"]) and not served[:, 3].any()
    print(flags, check_stride, "pairs:", want["pairs"].sum(), "robots near:", want["stats"]["robots_near"], "min:", want["stats"]["min_sep2"], want["stats"]["min_pair"])
    assert want["stats"]["robots_near"] >= 4 and (want["near_checks"] == 0).any()
    if flags == 3:
        stranded = np.isin(late["status"], (RM.OUT_OF_MAP, RM.NO_FIELD))
        assert (want["first_near_robot"] != want["min_sep_robot"]).any() and (want["partner_of"] & stranded).any()


# -- the statistics of a call: sep_fold over its check rows ----------------------------------------------------------------

def starts(n):
    """start ticks of a fleet: most robots leave at once, every fifth after 10 ticks, some after 1 or 40, one never"""
    if n == 2:
        return np.array([0, 3], np.uint32)
    st = np.zeros(n, np.uint32)
    st[::5] = 10
    st[1::7] = 1
    st[3::11] = 40
    st[2] = 1000
    return st


def converging_fleet(w, n):
    """n robots of which two are stranded beside the mesh (with_stranded) and at least a dozen head for the shared goal in
    the middle of the mesh, several per plan; n = 2: one of those and a second one that starts 5 cm beside it on the same plan.
    w: a world with `model` and `fleet(seed, per_family, drivers, close)` (tests/test_gpu_rollout.py's, or HostWorld)"""
    if n == 2:
        robots, goals = w.fleet(40, 0, 2, close=2)
        robots["pos"][1] = robots["pos"][0] + np.array([0, 0.05, 0], F32)
        robots["dir"][1], robots["slot"][1], robots["face_in"][1] = robots["dir"][0], robots["slot"][0], FM.NONE
        if robots.get("seed_face") is not None:
            robots["seed_face"][1] = robots["seed_face"][0]
    else:
        per_family = 3 if n == 65 else 9
        robots, goals = with_stranded(w.model, *w.fleet(40, per_family, n - 9 * per_family - 2, close=12 if n == 65 else 40))
    assert robots["pos"].shape[0] == n
    return robots, goals


class HostWorld:
    """what converging_fleet asks of a world, without a device: the three fields of build_world as the plans"""

    def __init__(self, model, fields, seed_faces):
        self.model, self.fields, self.seed_faces = model, fields, seed_faces

    def fleet(self, seed, per_family, drivers, close=5):
        return fleet(self.model, len(self.fields), self.seed_faces, seed, per_family, drivers, close)


FOLD_KEYS = ("checks_run", "checks_skipped", "first_skipped_tick", "robots_near", "near_pairs", "max_pairs", "max_pairs_tick", "min_pair", "tests", "max_cell")


def fold(L, chk, check_stride, near_checks, min_sep2, min_sep_robot):
    """sep_fold (the header's own) over check rows (k, 4) and the three columns; returns the statistics by name"""
    chk = np.ascontiguousarray(chk, np.uint64).reshape(-1, 4)
    near, m, who = np.ascontiguousarray(near_checks, np.uint32), np.ascontiguousarray(min_sep2, F32), np.ascontiguousarray(min_sep_robot, np.uint32)
    out, m_out = np.full(11, 99, np.uint64), np.zeros(1, F32)
    L.sep_fold_stats(_p(chk), chk.shape[0], check_stride, near.shape[0], _p(near), _p(m), _p(who), _p(out), _p(m_out))
    v = [int(x) for x in out]
    return dict(zip(FOLD_KEYS, v[:7] + [(v[7], v[8])] + v[9:]), min_sep2=m_out[0])


@pytest.fixture(scope="module")
def converging(built):
    """the converging fleets of tests/test_gpu_fleet_rollout.py on the host world and the model's run of each over TICKS
    ticks, computed once per n"""
    mesh, model, fields, seed_faces, start_face = built
    made = {}

    def get(n):
        if n not in made:
            robots, goals = converging_fleet(HostWorld(model, fields, seed_faces), n)
            made[n] = (robots, goals, starts(n), SM.departures(model, CONFIGS["default"], fields, robots, goals, DT, TICKS, DIST_TOL, ANG_TOL, starts(n)))
        return made[n]

    return get


@pytest.mark.parametrize("n,check_stride", [(2, 1), (2, 7), (65, 1), (65, 7)])
def test_the_fold_of_a_call_gives_the_models_statistics(world, converging, n, check_stride):
    model, fields, _, _, mirror, cfg, _, _ = world
    robots, goals, start, late = converging(n)
    want = SM.separation(late["trace"], late["status_at"], start, RADIUS, check_stride, 3)
    got = mirror.run_fleet(cfg, fields, robots, goals, TICKS, start_tick=start, radius=RADIUS, check_stride=check_stride, flags=3)
    SM.assert_same_rows(got, want, (n, check_stride))
    st = fold(mirror.L, got["chk"][: TICKS // check_stride], check_stride, got["near_checks"], got["min_sep2"], got["min_sep_robot"])
    for k in ("checks_run", "checks_skipped", "first_skipped_tick", "robots_near", "near_pairs", "max_pairs", "max_pairs_tick", "min_pair"):   # check_sep_stats' keys
        assert st[k] == want["stats"][k], (k, st, want["stats"])
    assert FM.same_bits(np.array([st["min_sep2"]], F32), np.array([want["stats"]["min_sep2"]], F32))
    assert want["stats"]["near_pairs"] > 0 and st["tests"] >= 2 * st["near_pairs"] and st["max_cell"] >= 1
    if n == 65:
        assert 0 < want["stats"]["robots_near"] < n and want["stats"]["max_pairs_tick"] > check_stride


def test_the_fold_of_tables_written_by_hand(shim):
    none = SM.NONE
    near, m, who = [0, 2, 1, 0], [np.inf, 0.25, 0.25, np.inf], [none, 2, 1, none]
    # a skipped check in the middle (rows: tests, ordered near pairs, largest cell, skipped): it counts, with its tick, and so
    # does its largest cell; its tests and pairs do not
    st = fold(shim, [[100, 6, 4, 0], [999999, 8, 50, 1], [30, 2, 3, 0]], 5, near, m, who)
    assert st == dict(checks_run=2, checks_skipped=1, first_skipped_tick=10, robots_near=2, near_pairs=4, max_pairs=3, max_pairs_tick=5, min_pair=(1, 2), tests=130,
                      max_cell=50, min_sep2=F32(0.25))
    # ... only the first skipped check gives the tick
    st = fold(shim, [[1, 0, 1, 1], [100, 6, 4, 0], [7, 0, 9, 1]], 5, near, m, who)
    assert (st["checks_run"], st["checks_skipped"], st["first_skipped_tick"], st["max_cell"], st["tests"], st["max_pairs_tick"]) == (1, 2, 5, 9, 100, 10)
    # two checks with the same number of pairs: the first keeps max_pairs_tick; the smallest index of the closest pair wins
    st = fold(shim, [[5, 2, 1, 0], [10, 4, 2, 0], [12, 4, 2, 0]], 3, near, m, who)
    assert (st["max_pairs"], st["max_pairs_tick"], st["near_pairs"], st["min_pair"]) == (2, 6, 5, (1, 2))
    # checks without a pair: the first one is the maximum; nobody near: the values of "never"
    st = fold(shim, [[3, 0, 1, 0], [3, 0, 1, 0]], 4, [0, 0], [np.inf, np.inf], [none, none])
    assert st == dict(checks_run=2, checks_skipped=0, first_skipped_tick=none, robots_near=0, near_pairs=0, max_pairs=0, max_pairs_tick=4, min_pair=(none, none), tests=6,
                      max_cell=1, min_sep2=F32(np.inf))
    # no check at all: the reset values
    st = fold(shim, np.zeros((0, 4)), 1, [0], [np.inf], [none])
    assert st == dict(checks_run=0, checks_skipped=0, first_skipped_tick=none, robots_near=0, near_pairs=0, max_pairs=0, max_pairs_tick=none, min_pair=(none, none), tests=0,
                      max_cell=0, min_sep2=F32(np.inf))
