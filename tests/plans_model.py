"""The rule of mnav_fleet_plans and mnav_fleet_walk_plans (include/mnav.h): the paths of
tests/fleet_model.py and the rows of OracleMesh.cvp_backtrack, posed by the CPU oracle's restatement of makePlan's pose
loops (OracleMesh.dijkstra_poses, OracleMesh.cvp_poses).  tests/test_plans_model.py pins the header's host mirror against
it; tests/test_gpu_fleet_plans.py pins the device."""
from __future__ import annotations

import numpy as np

from tests import fleet_model as FM


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(om, vn, fields, V, slots, vtx, start_pos, goal_pos):
    """the whole call: fleet_model.run's codes, potential and counts; path_len / offsets in poses; poses (total, 7) and
    cost per robot from OracleMesh.dijkstra_poses over each robot's ids"""
    base = FM.run(fields, V, slots, vtx)
    n = len(slots)
    lens, cost, rows = np.zeros(n, np.uint32), np.zeros(n, np.float64), []
    for i in range(n):
        lo, hops = int(base["offsets"][i]), int(base["path_len"][i])
        if hops:
            poses, cost[i] = om.dijkstra_poses(vn, base["ids"][lo: lo + hops], start_pos[i], goal_pos[int(slots[i])])
            assert poses.shape[0] == hops + 1
            rows.append(poses)
            lens[i] = hops + 1
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens.astype(np.uint64))
    poses = np.concatenate(rows) if rows else np.zeros((0, 7), np.float64)
    return dict(codes=base["codes"], potential=base["potential"], counts=base["counts"], path_len=lens, offsets=off, poses=poses, cost=cost)


def walk_run(om, fn, rows, slots, goal_pose):
    """rows[i] = (positions, faces) of robot i, seed first (OracleMesh.cvp_backtrack): path_len, offsets, poses, cost"""
    n = len(rows)
    lens, cost, out = np.zeros(n, np.uint32), np.zeros(n, np.float64), []
    for i, (ppos, pface) in enumerate(rows):
        if len(pface):
            poses, cost[i] = om.cvp_poses(fn, ppos, pface, goal_pose[int(slots[i])])
            assert poses.shape[0] == len(pface)
            out.append(poses)
            lens[i] = len(pface)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens.astype(np.uint64))
    return dict(path_len=lens, offsets=off, poses=np.concatenate(out) if out else np.zeros((0, 7), np.float64), cost=cost)


def same_poses(got, want, where):
    """bit for bit; a NaN matches any NaN (payload and sign are not compared).  Returns the number of poses with a NaN."""
    got, want = np.ascontiguousarray(got, np.float64).reshape(-1, 7), np.ascontiguousarray(want, np.float64).reshape(-1, 7)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (where, "NaN components differ")
    assert np.array_equal(bits64(got)[~nan], bits64(want)[~nan]), (where, np.flatnonzero((bits64(got) != bits64(want)) & ~nan)[:8])
    return int(nan.any(axis=1).sum())


def same(got, want, where):
    """a fleet_plans result against run(): everything but the poses is compared bit for bit; returns the NaN pose count"""
    for k in ("codes", "path_len", "offsets"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert np.array_equal(FM.bits(got["potential"]), FM.bits(want["potential"])), where
    assert np.array_equal(bits64(got["cost"]), bits64(want["cost"])), (where, "cost")
    return same_poses(got["poses"], want["poses"], where)


def quat_branch(pose_rows):
    """which branch of tf2's getRotation made each (non-NaN) quaternion, told from the result: the trace of the rotation
    matrix is 4 w^2 - 1, so trace > 0 <=> |w| > 1/2; otherwise the largest of |x|, |y|, |z| names the largest diagonal
    element.  Returns counts [trace, xx, yy, zz] (near the boundaries the count is approximate; the tests only need > 0)."""
    q = np.asarray(pose_rows, np.float64).reshape(-1, 7)[:, 3:]
    q = q[~np.isnan(q).any(axis=1)]
    tr = np.abs(q[:, 3]) > 0.5
    big = np.argmax(np.abs(q[:, :3]), axis=1)
    return [int(tr.sum())] + [int(((big == k) & ~tr).sum()) for k in range(3)]
