"""What the CPU and the GPU tests of the warm repair share (the tile-batch engine started from rewound fields, k_tb_warm; DESIGN.md
§3.11, §3.14): the batches and scenarios beyond those of tests/replan_model.py and tests/replan_each_model.py, both imported
unchanged, and the measure of a plan's kept / unkept frontier.

The tiling of the tile-batch engine is built inside the library, so the tests state the frontier in CELLS: the vertices that
are kept and have a neighbour that is not.  A tile owns at most tb_tile vertices; a frontier of more vertices than that cannot
lie inside one tile, so it crosses a tile boundary whatever the tiling -- kept values then sit in ghost slots of tiles that own
vertices that are not kept, which is the case k_tb_warm's ghost rule and wake-up word exist for."""
from __future__ import annotations

import numpy as np

from tests import replan_each_model as E
from tests import replan_model as R

OFF = 0.3
# the scenarios of tests/replan_model.py that mnav_replan_dijkstra_batch repairs (reason 0) and the GPU test runs warm: moved
# targets with no event, an edge-weight event, the offsets 0.3, 0, -0.2 and 1e9 (goal_dist = +inf in float32), an event beyond the
# cut (L == cut) followed by one next to the seed (only the seed kept), batches of 5 and -- across the 64-plan flag block -- 170 plans
BATCH_SCENARIOS = ("wall48", "wall48_offset0", "wall48_offset-0.2", "wall48_offset1e+09", "edges48", "beyond96", "targets48", "batch5", "batch170")
TB_TILE = {48: 64, 96: 120, 160: 120}      # option tb_tile of the GPU tests per terrain size (120: the default, the only one k_tbv_solve takes)


def frontier(N: int, keep) -> int:
    """kept vertices with a neighbour that is not kept"""
    adj = R.adjacency(N)
    return sum(1 for v in np.flatnonzero(keep) if any(not keep[u] for u, _ in adj[v]))


def tbv_batch():
    """terrain(160), the smallest mesh tests/test_gpu_tile_batch.py runs k_tbv_solve on: 96 plans, so that more than 64 are
    REPAIRED without the FRESH class, and one blocked 9 x 9 patch in the middle: (seeds, targets, patch ids)"""
    W = R.World(160, True)
    rng = np.random.default_rng(96)
    V = W.mesh.V
    s, t = rng.integers(0, V, 96), rng.integers(0, V, 96)
    t = np.where(t == s, (t + 7) % V, t)
    return s.tolist(), t.tolist(), W.rect(0.5, 0.5, 4)


def plan_facts(W, old, seeds, targets, offset, C, new_t, new_off, f):
    """per plan (class, L, cut, kept, rewound, reached, frontier) by the numpy rule on the old potentials"""
    out = []
    for p, s in enumerate(seeds):
        c, L, cut = E.classify(W.N, old[p].dist, targets[p], offset, C, new_t[p], new_off, f)
        keep = R.keep_mask(old[p].dist, L, s)
        fin = np.isfinite(old[p].dist)
        out.append((c, L, cut, int(keep.sum()), int((~keep & fin).sum()), int(fin.sum()), frontier(W.N, keep)))
    return out
