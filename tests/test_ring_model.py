"""The wait-for analysis of a yielding fleet rollout without a GPU: mesh_navigation_amd/csrc/mnav_fleet_ring.h compiled for the
host (g++ -ffp-contract=off, the flags of the library) -- the key, the doubling step and the classification are the device's
own source, ring_check_host composes them serially behind the check of mnav_fleet_yield.h -- against tests/ring_model.py, which
walks every chain with a visited set.  Point sets that pin every class, each at separation_cell_scale 1, 2 and 4 and with the
fewest rounds of the doubling, three more, and the early exit; rings and a convoy on a mesh through the whole call's host
mirror; and the fold of a call's check rows into its statistics (ring_fold).  Every comparison is exact."""
import ctypes as C
import itertools
import shutil
import subprocess

import numpy as np
import pytest

from tests import follow_model as FM
from tests import ring_model as RG
from tests import rollout_model as RM
from tests import separation_model as SM
from tests import yield_model as YM
from tests.test_follow_model import build_world
from tests.test_locate_model import CSRC
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT
from tests.test_separation_model import SCALES
from tests.test_yield_model import AHEAD_COS, RADIUS, SHIM as YIELD_SHIM, SLOW, YieldMirror, convoy, random_fleet

F32 = np.float32
NONE = SM.NONE
YROWS = ("hold_checks", "held_ticks", "first_hold_tick", "first_hold_robot")
RROWS = ("ring_checks", "first_ring_tick", "parked_checks", "released_checks", "wait_class", "wait_anchor")       # the order of mnav_frol::RRows

SHIM = YIELD_SHIM + r'''
#include "mnav_fleet_ring.h"

extern "C" uint32_t ring_launches(uint32_t n) { return mnav_frol::ring_launches(n); }
extern "C" uint32_t ring_rounds(uint32_t held, uint32_t launched, int early) { return mnav_frol::ring_rounds(held, launched, early != 0); }
// one check with the rule and the analysis: yld_check's arguments, then ring_flags, the rounds launched, the early exit, the
// six ring arrays (the order of mnav_frol::RRows) and rchk (kRingCheckWords).  Returns 1 when the pair pass ran
extern "C" int ring_check(uint32_t n, const float* pos, const float* dir, const int32_t* status, const uint32_t* start_tick, const uint32_t* priority, uint32_t tick,
                          uint32_t flags, float r, float scale, float c, uint32_t table_size, uint64_t max_tests, uint32_t* near_checks, uint32_t* max_partners,
                          uint32_t* first_near_tick, uint32_t* first_near_robot, float* min_sep2, uint32_t* min_sep_tick, uint32_t* min_sep_robot,
                          uint32_t* hold_checks, uint32_t* held_ticks, uint32_t* first_hold_tick, uint32_t* first_hold_robot, uint8_t* hold, uint64_t* chk, uint32_t* ychk,
                          uint32_t ring_flags, uint32_t launched, int early, uint32_t* ring_checks, uint32_t* first_ring_tick, uint32_t* parked_checks,
                          uint32_t* released_checks, uint8_t* wait_class, uint32_t* anchor, uint32_t* rchk)
{
  const mnav_frol::Rows A{ near_checks, max_partners, first_near_tick, first_near_robot, min_sep2, min_sep_tick, min_sep_robot };
  const mnav_frol::YRows Y{ hold_checks, held_ticks, first_hold_tick, first_hold_robot };
  const mnav_frol::RRows W{ ring_checks, first_ring_tick, parked_checks, released_checks, wait_class, anchor };
  return mnav_frol::ring_check_host(n, pos, dir, status, start_tick, priority, tick, flags, mnav_frol::sep_grid(r, scale), c * c, table_size, max_tests, A, Y, hold, chk,
                                    ychk, ring_flags, launched, early != 0, W, rchk) ? 1 : 0;
}
// yrol_batch with the analysis behind every check: its arguments, then ring_flags, the early exit, the six ring arrays and rchk
// (kRingCheckWords per check).  The rounds launched are ring_launches(n), the device's.
extern "C" void rrol_batch(void* h, uint32_t n, const uint32_t* slot, const uint32_t* seed_face, const float* goal_pos, const float* goal_dir, const float* fields,
                           const float* costs, const double* cfg, const double* par, uint32_t ticks, uint32_t stride, uint32_t V, uint32_t F, const float* xyz,
                           const uint32_t* faces, const uint32_t* vf_ptr, const uint32_t* vf, int32_t* status, uint32_t* tk, float* pos, float* dir,
                           const float* up, uint32_t* face, double* travel, double* cost_integral, float* min_goal_dist, float* trace, uint64_t* how,
                           const uint32_t* start_tick, float r, float scale, uint32_t check_stride, uint32_t flags, uint64_t max_tests, uint32_t* near_checks,
                           uint32_t* max_partners, uint32_t* first_near_tick, uint32_t* first_near_robot, float* min_sep2, uint32_t* min_sep_tick,
                           uint32_t* min_sep_robot, uint64_t* chk, float c, const uint32_t* priority, uint8_t* hold, uint32_t* hold_checks, uint32_t* held_ticks,
                           uint32_t* first_hold_tick, uint32_t* first_hold_robot, uint32_t* ychk, uint32_t ring_flags, int early, uint32_t* ring_checks,
                           uint32_t* first_ring_tick, uint32_t* parked_checks, uint32_t* released_checks, uint8_t* wait_class, uint32_t* anchor, uint32_t* rchk)
{
  Host* H = (Host*)h;
  const Index I{ H->nodes.data(), H->pts.data(), H->n_pts, H->n_leaves, loc_root(H->n_leaves) };
  const mnav::WalkMesh Mh{ xyz, faces, vf_ptr, vf, V, F };
  mnav_fol::Config Cf;
  std::memcpy(&Cf, cfg, sizeof(Cf));
  const mnav_rol::Params P = params(par, goal_pos != nullptr);
  const ::Rows A{ status, tk, pos, dir, up, face, travel, cost_integral, min_goal_dist };
  const mnav_frol::Rows S{ near_checks, max_partners, first_near_tick, first_near_robot, min_sep2, min_sep_tick, min_sep_robot };
  const mnav_frol::YRows Y{ hold_checks, held_ticks, first_hold_tick, first_hold_robot };
  const mnav_frol::RRows W{ ring_checks, first_ring_tick, parked_checks, released_checks, wait_class, anchor };
  VecStack st; st.cap = kStack;
  std::vector<uint32_t> list(mnav::kWalkScratchWords);
  const uint32_t rows = stride ? ticks / stride : 0;
  const mnav::W3 zero = mnav::w3(0, 0, 0);
  for (uint32_t t = 1; t <= ticks; ++t) {
    for (uint32_t i = 0; i < n; ++i) {
      const bool waits = start_tick && mnav_frol::frol_waits(t, start_tick[i]);
      if (!waits && !hold[i]) {
        const mnav::WalkField Fd = mnav_fol::fol_field(Mh, fields + 3 * (size_t)V * slot[i], seed_face ? seed_face[i] : mnav::kNone);
        State R = load(A, i);
        mnav_rol::rol_run(Mh, I, st, Fd, costs, Cf, P, goal_pos ? mnav::w3_load(goal_pos + 3 * (size_t)i) : zero, goal_dir ? mnav::w3_load(goal_dir + 3 * (size_t)i) : zero,
                          R, 1, 0, nullptr, list.data(), how);
        store(A, i, R);
      } else if (mnav_frol::yld_mover(status[i], waits)) held_ticks[i] += 1;
      if (stride && t % stride == 0) std::memcpy(trace + 3 * ((size_t)rows * i + t / stride - 1), pos + 3 * (size_t)i, 12);
    }
    if (t % check_stride == 0) {
      const uint32_t k = t / check_stride - 1;
      mnav_frol::ring_check_host(n, pos, dir, status, start_tick, priority, t, flags, mnav_frol::sep_grid(r, scale), c * c, mnav_frol::sep_table_size(n), max_tests, S, Y,
                                 hold, chk + (size_t)mnav_frol::kCheckWords * k, ychk + (size_t)mnav_frol::kYldCheckWords * k, ring_flags, mnav_frol::ring_launches(n),
                                 early != 0, W, rchk + (size_t)mnav_frol::kRingCheckWords * k);
    }
  }
}
// ring_fold over the rows of `checks` checks and one of the robots' columns; out: robots_ring, rings, max_rings, max_rings_tick,
// releases, members / tails / parked / queued / rings at the last check, checks_run, checks_skipped, first_skipped_tick, (13)
// what the fold must leave alone: the four times
extern "C" void ring_fold_stats(const uint64_t* chk, const uint32_t* rchk, uint32_t checks, uint32_t check_stride, uint32_t n, const uint32_t* ring_checks, uint64_t* out)
{
  mnav_frol::RingStats S;
  mnav_frol::ring_fold(chk, rchk, checks, check_stride, n, ring_checks, S);
  out[0] = S.robots_ring; out[1] = S.rings; out[2] = S.max_rings; out[3] = S.max_rings_tick; out[4] = S.releases; out[5] = S.members_last; out[6] = S.tails_last;
  out[7] = S.parked_last; out[8] = S.queued_last; out[9] = S.rings_last; out[10] = S.checks_run; out[11] = S.checks_skipped; out[12] = S.first_skipped_tick;
  out[13] = (S.ms_ring != 0.f) + (S.ms_separation != 0.f) + (S.ms_kernels != 0.f) + (S.ms_total != 0.f);
}
'''
STAT_KEYS = ("robots_ring", "rings", "max_rings", "max_rings_tick", "releases", "members_last", "tails_last", "parked_last", "queued_last", "rings_last", "checks_run",
             "checks_skipped", "first_skipped_tick")


def build_shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_fleet_ring.h"
    d = tmp_path_factory.mktemp("ring_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    L.loc_build.restype = vp
    L.loc_build.argtypes = [u32, vp]
    L.loc_free.argtypes = [vp]
    L.sep_table_size.restype = u32
    L.sep_table_size.argtypes = [u32]
    L.ring_launches.restype = u32
    L.ring_launches.argtypes = [u32]
    L.ring_rounds.restype = u32
    L.ring_rounds.argtypes = [u32, u32, C.c_int]
    L.yrol_batch.argtypes = [vp, u32] + [vp] * 8 + [u32] * 4 + [vp] * 15 + [vp, f32, f32, u32, u32, C.c_uint64] + [vp] * 8 + [f32] + [vp] * 7
    L.ring_check.restype = C.c_int
    L.ring_check.argtypes = [u32] + [vp] * 5 + [u32, u32, f32, f32, f32, u32, C.c_uint64] + [vp] * 14 + [u32, u32, C.c_int] + [vp] * 7
    L.rrol_batch.argtypes = L.yrol_batch.argtypes + [u32, C.c_int] + [vp] * 7
    L.ring_fold_stats.argtypes = [vp, vp, u32, u32, u32, vp, vp]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


Z = np.array([0, 0, 1], F32)


def fewest_rounds(held):
    """the smallest k with 2^k >= held"""
    return 0 if held <= 1 else int(held - 1).bit_length()


def host_check(L, pos, direction, radius, ahead_cos, scale, status, start_tick, priority, tick, flags, ring_flags, launched, early, max_tests=2 ** 63):
    n = pos.shape[0]
    rows, yrows, rrows = SM.start_rows(n), YM.start_yrows(n), RG.start_rrows(n)
    rrows["wait_class"][:], rrows["wait_anchor"][:] = 9, 9            # every entry is written
    st = None if start_tick is None else np.ascontiguousarray(start_tick, np.uint32)
    pr = None if priority is None else np.ascontiguousarray(priority, np.uint32)
    hold, chk, ychk, rchk = np.full(n, 9, np.uint8), np.zeros(4, np.uint64), np.full(1, 99, np.uint32), np.full(6, 99, np.uint32)
    ran = L.ring_check(n, _p(pos), _p(direction), _p(status), _p(st), _p(pr), tick, flags, radius, scale, ahead_cos, L.sep_table_size(n), max_tests,
                       *[_p(rows[k]) for k in SM.SEP_KEYS], *[_p(yrows[k]) for k in YROWS], _p(hold), _p(chk), _p(ychk), ring_flags, launched, int(early),
                       *[_p(rrows[k]) for k in RROWS], _p(rchk))
    return rows, yrows, rrows, hold, chk, int(ychk[0]), dict(zip(RG.COUNT_KEYS, (int(v) for v in rchk))), bool(ran)


def both(L, pos, direction, radius=0.3, ahead_cos=0.5, status=None, start_tick=None, priority=None, tick=1, flags=0, ring_flags=0, what="", scales=SCALES):
    """one check by the model and by the header -- at every scale, with the fewest rounds that cover the robots held, with
    three more, and with the device's rounds and the early exit: equal.  Returns the model's (hold, hold0, blocker, counts,
    rrows)"""
    pos, direction = np.ascontiguousarray(pos, F32).reshape(-1, 3), np.ascontiguousarray(direction, F32).reshape(-1, 3)
    n = pos.shape[0]
    status = np.zeros(n, np.int32) if status is None else np.ascontiguousarray(status, np.int32)
    waiting = np.zeros(n, bool) if start_tick is None else tick <= np.asarray(start_tick, np.int64)
    rows, yrows, rrows = SM.start_rows(n), YM.start_yrows(n), RG.start_rrows(n)
    hold, hold0, b, counts = RG.check(rows, yrows, rrows, pos, direction, status, waiting, flags, radius, ahead_cos, priority, tick, ring_flags)
    k = fewest_rounds(int(hold0.sum()))
    assert L.ring_rounds(int(hold0.sum()), L.ring_launches(n), 1) == k <= L.ring_launches(n) == max(fewest_rounds(n), 1)
    for scale in scales:
        for launched, early in ((k, False), (k + 3, False), (L.ring_launches(n), True)):
            g_rows, g_yrows, g_rrows, g_hold, chk, held, g_counts, ran = host_check(L, pos, direction, radius, ahead_cos, scale, status, start_tick, priority, tick,
                                                                                   flags, ring_flags, launched, early)
            where = (what, scale, launched, early)
            assert ran and held == int(hold0.sum()) and g_counts == counts, (where, held, g_counts, counts)
            SM.assert_same_rows(g_rows, rows, where)
            YM.assert_same_yield(dict(g_yrows, hold=g_hold), dict(yrows, hold=hold), where)
            RG.assert_same_rings(g_rrows, rrows, where)
    return hold, hold0, b, counts, rrows


def circle(n, spacing=0.2, centre=(0.0, 0.0, 0.0), heading="tangent", phase=0.0):
    """n robots on a circle, neighbours `spacing` apart, counter-clockwise from the angle `phase`: robot i + 1 is ahead of
    robot i.  heading: along the tangent, or for the next robot"""
    a = phase + 2 * np.pi * np.arange(n) / n
    rad = spacing / (2 * np.sin(np.pi / n))
    pos = np.array(centre)[None, :] + rad * np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1)
    if heading == "tangent":
        d = np.stack([-np.sin(a), np.cos(a), np.zeros(n)], axis=1)
    else:
        d = np.roll(pos, -1, axis=0) - pos
        d /= np.linalg.norm(d, axis=1)[:, None]
    return pos.astype(F32), d.astype(F32)


def line(n, spacing=0.2, origin=(0.0, 0.0, 0.0), towards=(1.0, 0.0, 0.0)):
    """n robots on a line heading along it, the LAST one in front: robot i + 1 is ahead of robot i"""
    u = np.array(towards, np.float64)
    pos = np.array(origin)[None, :] + spacing * np.arange(n)[:, None] * u[None, :]
    return pos.astype(F32), np.tile(u.astype(F32), (n, 1))


def ring_with_tail(ring=5, tail=3, spacing=0.2, phase=0.0):
    """a ring of `ring` robots and `tail` robots on the radial line through robot 0, outside, heading for it"""
    pos, d = circle(ring, spacing, phase=phase)
    out = pos[0].astype(np.float64) / np.linalg.norm(pos[0])
    tpos = np.array([pos[0] + spacing * (k + 1) * out for k in range(tail)], F32)
    return np.concatenate([pos, tpos]), np.concatenate([d, np.tile((-out).astype(F32), (tail, 1))])


# -- single checks ---------------------------------------------------------------------------------------------------------

def test_a_triangle_under_all_priority_orders(shim):
    """each robot heads for the next (cosine 0.9: the robot ahead sees its follower 60 degrees off its heading, outside the
    cone): a ring of three, the smallest there is, whose leader follows (priority, index)"""
    pos, d = circle(3, heading="next")
    orders = [None, [4, 4, 4]] + [list(p) for p in itertools.permutations((0, 1, 2))] + [[1, 0, 0], [0, 1, 0], [7, 7, 3]]
    for prio in orders:
        for ring_flags in (0, RG.RELEASE):
            hold, hold0, b, counts, r = both(shim, pos, d, 0.3, 0.9, priority=prio, tick=5, ring_flags=ring_flags, what=("triangle", prio, ring_flags))
            leader = min(range(3), key=lambda i: ((prio or [0] * 3)[i], i))
            assert hold0.tolist() == [1, 1, 1] and b.tolist() == [1, 2, 0]
            assert r["wait_class"].tolist() == [RG.RING_MEMBER] * 3 and r["wait_anchor"].tolist() == [leader] * 3
            assert counts == dict(queued=0, parked=0, tails=0, members=3, rings=1, released=1 if ring_flags else 0)
            assert hold.tolist() == [0 if ring_flags and i == leader else 1 for i in range(3)]
            assert r["released_checks"].tolist() == [1 if ring_flags and i == leader else 0 for i in range(3)]
            assert r["ring_checks"].tolist() == [1] * 3 and r["first_ring_tick"].tolist() == [5] * 3
    # tangent headings: the next robot sits exactly on the cone of 60 degrees, so the cone is opened to cosine 0.25
    pos, d = circle(3)
    hold, hold0, b, counts, r = both(shim, pos, d, 0.3, 0.25, what="tangent triangle")
    assert b.tolist() == [1, 2, 0] and counts["members"] == 3


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 128, 129, 257])
def test_rings_on_a_circle(shim, n):
    pos, d = circle(n)
    prio = ((np.arange(n) * 5 + 2) % 3).astype(np.uint32)
    for priority, leader in ((None, 0), (prio, int(np.lexsort((np.arange(n), prio))[0]))):
        for ring_flags in (0, RG.RELEASE):
            hold, hold0, b, counts, r = both(shim, pos, d, 0.3, 0.25 if n == 3 else 0.5, priority=priority, ring_flags=ring_flags, what=("ring", n),
                                             scales=SCALES if n <= 65 else (2.0,))
            assert hold0.all() and np.array_equal(b, (np.arange(n) + 1) % n)                       # (the construction: everybody behind the next)
            assert (r["wait_class"] == RG.RING_MEMBER).all() and (r["wait_anchor"] == leader).all()
            assert counts == dict(queued=0, parked=0, tails=0, members=n, rings=1, released=1 if ring_flags else 0)
            assert int(hold.sum()) == n - (1 if ring_flags else 0) and hold[leader] == (0 if ring_flags else 1)


def test_a_ring_of_five_with_a_tail_of_three(shim):
    pos, d = ring_with_tail()
    for prio, leader in ((None, 0), ([3, 3, 1, 3, 3, 0, 0, 0], 2)):
        hold, hold0, b, counts, r = both(shim, pos, d, priority=prio, ring_flags=RG.RELEASE, what=("tail", prio))
        assert b.tolist() == [1, 2, 3, 4, 0, 0, 5, 6] and hold0.all()
        assert r["wait_class"].tolist() == [RG.RING_MEMBER] * 5 + [RG.RING_TAIL] * 3 and r["wait_anchor"].tolist() == [leader] * 8          # one anchor
        assert counts == dict(queued=0, parked=0, tails=3, members=5, rings=1, released=1)
        assert hold.tolist() == [0 if i == leader else 1 for i in range(8)]                    # the tail stays held, whatever its priorities
        assert r["ring_checks"].tolist() == [1] * 5 + [0] * 3 and r["first_ring_tick"].tolist() == [1] * 5 + [NONE] * 3


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 9, 10, 17, 18, 33, 34, 65, 66, 129, 130])
def test_a_line_behind_a_mover_and_behind_a_parked_robot(shim, n):
    """depth n - 1: the powers of two and one more are where the doubling is off by one if it is"""
    pos, d = line(n)
    want_b = np.append(np.arange(1, n), NONE).astype(np.uint32)
    scales = SCALES if n <= 34 else (2.0,)
    hold, hold0, b, counts, r = both(shim, pos, d, what=("queued", n), scales=scales)
    assert np.array_equal(b, want_b) and int(hold0.sum()) == n - 1
    assert r["wait_class"].tolist() == [RG.QUEUED] * (n - 1) + [RG.FREE] and r["wait_anchor"].tolist() == [n - 1] * (n - 1) + [NONE]
    assert counts == dict(queued=n - 1, parked=0, tails=0, members=0, rings=0, released=0)
    # the head has not departed and is kept present: the same queue is parked
    start = np.zeros(n, np.uint32)
    start[n - 1] = 50
    for kw in (dict(start_tick=start, flags=SM.WAITING_PRESENT), dict(status=[RM.RUNNING] * (n - 1) + [RM.REACHED], flags=SM.REACHED_PRESENT),
               dict(status=[RM.RUNNING] * (n - 1) + [RM.NO_FIELD])):
        hold, hold0, b, counts, r = both(shim, pos, d, tick=3, ring_flags=RG.RELEASE, what=("parked", n, sorted(kw)), scales=scales, **kw)
        assert np.array_equal(b, want_b) and np.array_equal(hold, hold0)                     # nothing to release
        assert r["wait_class"].tolist() == [RG.PARKED] * (n - 1) + [RG.FREE] and r["wait_anchor"].tolist() == [n - 1] * (n - 1) + [NONE]
        assert counts == dict(queued=0, parked=n - 1, tails=0, members=0, rings=0, released=0) and r["parked_checks"].tolist() == [1] * (n - 1) + [0]


def mixed_fleet():
    """a ring of 67 (it crosses a wave), a triangle, a ring of 5 with its tail, a parked line of 33 and a queue of 9, apart"""
    parts = [circle(67, centre=(0, 0, 0)), circle(3, centre=(10, 0, 0), heading="next"), ring_with_tail(), line(34, origin=(0, 10, 0)), line(10, origin=(0, 12, 0))]
    parts[2] = (parts[2][0] + np.array([20, 0, 0], F32), parts[2][1])
    pos, d = np.concatenate([p for p, _ in parts]), np.concatenate([q for _, q in parts])
    status = np.zeros(pos.shape[0], np.int32)
    status[67 + 3 + 8 + 33] = RM.OUT_OF_MAP
    return pos, d, status


def test_every_class_in_one_check(shim):
    pos, d, status = mixed_fleet()
    n = pos.shape[0]
    prio = ((np.arange(n) * 7 + 3) % 4).astype(np.uint32)
    for priority in (None, prio):
        for ring_flags in (0, RG.RELEASE):
            # cosine 0.6: inside the cone of the tangent rings (the next robot is at most 36 degrees off), outside for the followers of the triangle (60 degrees)
            hold, hold0, b, counts, r = both(shim, pos, d, 0.3, 0.6, status=status, priority=priority, ring_flags=ring_flags, what=("mixed", ring_flags))
            assert counts == dict(queued=9, parked=33, tails=3, members=67 + 3 + 5, rings=3, released=3 if ring_flags else 0), counts
            assert int(hold0.sum()) - int(hold.sum()) == counts["released"]
            assert len(set(r["wait_anchor"][r["wait_class"] >= RG.RING_TAIL].tolist())) == 3


def test_257_random_robots(shim):
    rng = np.random.default_rng(21)
    seen = np.zeros(5, np.int64)
    for trial, (c, flags) in enumerate(((0.5, 3), (0.0, 0), (0.95, 1))):
        pos, d, status, start, prio = random_fleet(rng)
        for priority in (prio, None):
            hold, hold0, b, counts, r = both(shim, pos, d, 0.25, c, status=status, start_tick=start, priority=priority, tick=10, flags=flags, ring_flags=RG.RELEASE,
                                             what=("random", trial))
            print(trial, counts)
            seen += np.bincount(r["wait_class"], minlength=5)
            assert counts["queued"] + counts["parked"] + counts["tails"] + counts["members"] == int(hold0.sum()) > 10
    assert seen[RG.FREE] and seen[RG.QUEUED] and seen[RG.PARKED]


def test_a_skipped_check_leaves_every_class_free(shim):
    pos, d = circle(5)
    for scale in SCALES:
        rows, yrows, rrows, hold, chk, held, counts, ran = host_check(shim, pos, d, 0.3, 0.5, scale, np.zeros(5, np.int32), None, None, 1, 0, RG.RELEASE, 3, True, max_tests=3)
        assert not ran and int(chk[3]) == 1 and not hold.any() and held == 0 and counts == dict.fromkeys(RG.COUNT_KEYS, 0)
        RG.assert_same_rings(rrows, RG.start_rrows(5), "skipped")
        YM.assert_same_yield(dict(yrows, hold=hold), dict(YM.start_yrows(5), hold=np.zeros(5, np.uint8)), "skipped")
    assert host_check(shim, pos, d, 0.3, 0.5, 2.0, np.zeros(5, np.int32), None, None, 1, 0, 0, 3, True)[6]["members"] == 5


# -- the statistics of a call: ring_fold over its check rows ---------------------------------------------------------------

def fold(L, chk, rchk, check_stride, ring_checks):
    chk, rchk = np.ascontiguousarray(chk, np.uint64).reshape(-1, 4), np.ascontiguousarray(rchk, np.uint32).reshape(-1, 6)
    rc = np.ascontiguousarray(ring_checks, np.uint32)
    out = np.full(14, 99, np.uint64)
    L.ring_fold_stats(_p(chk), _p(rchk), chk.shape[0], check_stride, rc.shape[0], _p(rc), _p(out))
    assert out[13] == 0                                               # the fold leaves the times alone
    return dict(zip(STAT_KEYS, (int(v) for v in out[:13])))


def test_the_fold_of_tables_written_by_hand(shim):
    # separation rows: tests, ordered near pairs, largest cell, skipped; ring rows: queued, parked, tails, members, rings, released
    st = fold(shim, [[9, 2, 1, 0], [9, 2, 1, 1], [9, 2, 1, 0], [9, 2, 1, 0]], [[1, 2, 3, 8, 2, 2], [7, 7, 7, 7, 7, 7], [0, 1, 0, 9, 2, 0], [4, 3, 2, 5, 1, 1]], 5, [0, 3, 1, 0])
    assert st == dict(robots_ring=2, rings=5, max_rings=2, max_rings_tick=5, releases=3, members_last=5, tails_last=2, parked_last=3, queued_last=4, rings_last=1,
                      checks_run=3, checks_skipped=1, first_skipped_tick=10)
    # a later check with more rings takes the maximum; a skipped last check gives zeros at the last check
    st = fold(shim, [[9, 2, 1, 0], [9, 2, 1, 0], [9, 2, 1, 1]], [[0, 0, 0, 3, 1, 0], [0, 0, 0, 8, 2, 0], [5, 5, 5, 5, 5, 5]], 4, [2, 2])
    assert (st["max_rings"], st["max_rings_tick"], st["rings"], st["members_last"], st["rings_last"], st["first_skipped_tick"]) == (2, 8, 3, 0, 0, 12)
    none = dict(robots_ring=0, rings=0, max_rings=0, max_rings_tick=NONE, releases=0, members_last=0, tails_last=0, parked_last=0, queued_last=0, rings_last=0,
                checks_run=0, checks_skipped=0, first_skipped_tick=NONE)
    assert fold(shim, np.zeros((0, 4)), np.zeros((0, 6)), 1, [0, 0]) == none
    assert fold(shim, [[1, 0, 1, 1]], [[1, 1, 1, 1, 1, 1]], 3, [0]) == dict(none, checks_skipped=1, first_skipped_tick=3)
    assert fold(shim, [[1, 0, 1, 0]], [[0, 0, 0, 0, 0, 0]], 3, [0]) == dict(none, checks_run=1, max_rings_tick=3)


# -- on a mesh: the whole call ------------------------------------------------------------------------------------------

def place(model, xy, slot=2, seed_face=None, holes=False):
    """robots exactly on the mesh at the points xy: the face that holds the point and its barycentric z.  holes: a point over
    a hole of the mesh is no error: the robot has no face yet and the height of the nearest vertex"""
    xyz, faces = model.xyz.astype(np.float64), model.faces
    a, b, c = (xyz[faces[:, k]] for k in range(3))
    pos, face = [], []
    for q in np.asarray(xy, np.float64):
        den = (b[:, 1] - c[:, 1]) * (a[:, 0] - c[:, 0]) + (c[:, 0] - b[:, 0]) * (a[:, 1] - c[:, 1])
        with np.errstate(all="ignore"):
            u = ((b[:, 1] - c[:, 1]) * (q[0] - c[:, 0]) + (c[:, 0] - b[:, 0]) * (q[1] - c[:, 1])) / den
            v = ((c[:, 1] - a[:, 1]) * (q[0] - c[:, 0]) + (a[:, 0] - c[:, 0]) * (q[1] - c[:, 1])) / den
        inside = np.nonzero((u >= 0) & (v >= 0) & (u + v <= 1))[0]
        assert inside.size or holes, q
        if not inside.size:
            near = int(np.nanargmin((xyz[:, 0] - q[0]) ** 2 + (xyz[:, 1] - q[1]) ** 2))
            pos.append([q[0], q[1], xyz[near, 2]])
            face.append(FM.NONE)
            continue
        f = int(inside[0])
        pos.append([q[0], q[1], u[f] * a[f, 2] + v[f] * b[f, 2] + (1 - u[f] - v[f]) * c[f, 2]])
        face.append(f)
    n = len(pos)
    return dict(pos=np.array(pos, F32), up=np.tile(Z, (n, 1)), face_in=np.array(face, np.uint32), slot=np.full(n, slot, np.uint32),
                seed_face=None if seed_face is None else np.full(n, seed_face, np.uint32))


def ring_on_mesh(model, n, centre, spacing=0.2, slot=2, seed_face=None):
    pos, d = circle(n, spacing, centre=(centre[0], centre[1], 0.0))
    return dict(place(model, pos[:, :2], slot, seed_face), dir=d)


class RingMirror(YieldMirror):
    def run_rings(self, cfg, fields, robots, goals, ticks, start_tick=None, radius=RADIUS, scale=2.0, check_stride=1, flags=0, ahead_cos=AHEAD_COS, priority=None,
                  hold_in=None, max_tests=2 ** 63, ring_flags=0, early=True):
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
        trace, how = np.zeros((n, ticks, 3), F32), np.zeros(5, np.uint64)
        st = None if start_tick is None else np.ascontiguousarray(start_tick, np.uint32)
        pr = None if priority is None else np.ascontiguousarray(priority, np.uint32)
        rows, yrows, rrows = SM.start_rows(n), YM.start_yrows(n), RG.start_rrows(n)
        hold = np.zeros(n, np.uint8) if hold_in is None else (np.asarray(hold_in) != 0).astype(np.uint8)
        checks = max(ticks // check_stride, 1)
        chk, ychk, rchk = np.zeros((checks, 4), np.uint64), np.zeros(checks, np.uint32), np.zeros((checks, 6), np.uint32)
        self.L.rrol_batch(self.h, n, _p(slot), _p(sf), _p(gp), _p(gd), _p(fl), _p(m.costs), _p(c), _p(par), ticks, 1, m.V, m.F, _p(m.xyz),
                          _p(m.faces), _p(self.ptr), _p(self.vf), _p(S["status"]), _p(S["ticks"]), _p(S["pos"]), _p(S["dir"]), _p(upv), _p(S["face"]),
                          _p(S["travel"]), _p(S["cost_integral"]), _p(S["min_goal_dist"]), _p(trace), _p(how), _p(st), radius, scale, check_stride, flags,
                          max_tests, *[_p(rows[k]) for k in SM.SEP_KEYS], _p(chk), ahead_cos, _p(pr), _p(hold), *[_p(yrows[k]) for k in YROWS], _p(ychk),
                          ring_flags, int(early), *[_p(rrows[k]) for k in RROWS], _p(rchk))
        return dict(S, trace=trace, how=how.astype(np.int64), **rows, **yrows, **rrows, hold=hold, chk=chk, ychk=ychk, rchk=rchk)


def assert_equals_model(L, got, want, check_stride, what):
    RM.assert_same(got, want, (what, "state"))
    SM.assert_same_rows(got, want, (what, "separation"))
    YM.assert_same_yield(got, want, (what, "yield"))
    RG.assert_same_rings(got, want, (what, "rings"))
    checks = len(want["counts"])
    assert [dict(zip(RG.COUNT_KEYS, (int(v) for v in row))) for row in got["rchk"][:checks]] == want["counts"], what
    st = fold(L, got["chk"][:checks], got["rchk"][:checks], check_stride, got["ring_checks"])
    assert st == want["ring_stats"], (what, st, want["ring_stats"])


@pytest.fixture(scope="module")
def world(shim):
    mesh, model, fields, seed_faces, start_face = build_world("terrain")
    mirror = RingMirror(shim, model)
    yield model, fields, seed_faces, start_face, mirror
    mirror.close()


RING_TICKS = 120


@pytest.mark.parametrize("n", [5, 12])
def test_a_ring_on_the_terrain_persists_and_a_release_dissolves_it(world, n):
    """every robot of a ring on the mesh starts held (hold_in): without the release the first check finds the ring as it was
    placed and every later check finds it again; with it the leader drives off and the last check finds no ring"""
    model, fields, seed_faces, start_face, mirror = world
    mid = np.nanmean(model.xyz.astype(np.float64), axis=0)
    robots = ring_on_mesh(model, n, (mid[0] + 1.3, mid[1] + 0.9), seed_face=seed_faces[2])
    hold_in = np.ones(n, np.uint8)
    runs = {}
    for ring_flags in (0, RG.RELEASE):
        want = RG.run(model, SLOW, fields, robots, None, DT, RING_TICKS, DIST_TOL, ANG_TOL, None, RADIUS, 1, 0, AHEAD_COS, None, hold_in, ring_flags)
        runs[ring_flags] = want
        for scale, early in ((2.0, True), (1.0, False), (4.0, True)):
            got = mirror.run_rings(SLOW, fields, robots, None, RING_TICKS, scale=scale, hold_in=hold_in, ring_flags=ring_flags, early=early)
            assert_equals_model(mirror.L, got, want, 1, (n, ring_flags, scale, early))
    # conditions on the MODEL's output
    kept, freed = runs[0], runs[RG.RELEASE]
    assert (kept["class_at"] == RG.RING_MEMBER).all() and kept["ring_stats"]["rings"] == RING_TICKS and not kept["had_tick"].any()       # a ring that persists
    assert (kept["held_ticks"] == RING_TICKS).all() and kept["ring_stats"]["members_last"] == n
    gone = np.nonzero([c["rings"] == 0 for c in freed["counts"]])[0]
    print(n, "ring gone after", gone[0], "checks; last check:", freed["counts"][-1], "released:", freed["released_checks"])
    assert gone.size and freed["counts"][-1]["rings"] == 0 and freed["ring_stats"]["rings"] < RING_TICKS       # a ring that dissolves: absent at the last check
    first = np.array([np.nonzero(freed["class_at"][:, i] == RG.RING_MEMBER)[0][0] for i in range(n)])
    assert (first == 0).all() and (freed["first_ring_tick"] == 1).all()
    led = np.nonzero(freed["released_checks"])[0]
    assert led.size and all(freed["had_tick"][i, 1:].any() for i in led)                         # a released robot later has a tick
    assert freed["stats"]["held_ticks"] < kept["stats"]["held_ticks"] and freed["ring_stats"]["releases"] >= 1
    # hold_checks counts what the rule decided, released or not; held_ticks what the flags left
    i = int(led[0])
    assert freed["hold_checks"][i] > freed["held_at"][:, i].sum()


def test_the_convoy_with_the_analysis_is_the_convoy_without(world):
    """flags 0: state, separation and yield outputs of yield_model.run; with the release: ring_model.run (a convoy has no ring,
    so the release changes nothing either -- the classes tell a queue from a parked queue)"""
    model, fields, seed_faces, start_face, mirror = world
    robots, goals, gaps = convoy(model, fields, seed_faces, start_face, SLOW)
    start = np.array([0, 0, 0, 0, 4, 9], np.uint32)
    for stride, flags in ((1, 0), (7, 3)):
        plain = YM.run(model, SLOW, fields, robots, goals, DT, 120, DIST_TOL, ANG_TOL, start, RADIUS, stride, flags, AHEAD_COS)
        got = mirror.run_rings(SLOW, fields, robots, goals, 120, start_tick=start, check_stride=stride, flags=flags)
        RM.assert_same(got, plain, "state")
        SM.assert_same_rows(got, plain, "separation")
        YM.assert_same_yield(got, plain, "yield")
        assert np.array_equal(got["ychk"][: 120 // stride], plain["held_at"].sum(axis=1))
        same = mirror.run_yield(SLOW, fields, robots, goals, 120, start_tick=start, check_stride=stride, flags=flags)
        assert all(FM.same_bits(np.asarray(got[k]), np.asarray(same[k])) for k in same)            # the mirror of the call without the analysis, every array
        want = RG.run(model, SLOW, fields, robots, goals, DT, 120, DIST_TOL, ANG_TOL, start, RADIUS, stride, flags, AHEAD_COS, None, None, RG.RELEASE)
        got = mirror.run_rings(SLOW, fields, robots, goals, 120, start_tick=start, check_stride=stride, flags=flags, ring_flags=RG.RELEASE)
        assert_equals_model(mirror.L, got, want, stride, ("convoy", stride))
        seen = np.bincount(want["class_at"].reshape(-1), minlength=5)
        print(stride, flags, "classes over the call:", seen, want["ring_stats"])
        assert seen[RG.QUEUED] and seen[RG.RING_MEMBER] == 0 and (flags == 0 or seen[RG.PARKED])
