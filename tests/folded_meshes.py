"""The folded and closed meshes the CPU and the GPU tests share (meshgen.ramp / torus / tube / moved), their tilings on the
tile-batch engine, and the plans that end on the late ghosts of a long slice.

A tile's slice is its T owned slots and then its ghosts, ordered by (owner tile, local index).  On the ramp a tile is a column
through every storey, so it has several small patches and a rim of ghosts around each: most slices are longer than 256 slots, and
the ghosts of a tile's last neighbours sit in the slots from 256 on ("late" ghosts: ghost index >= 256 - T)."""
from __future__ import annotations

import functools

import numpy as np

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests import replan_model as R
from tests.common import Case

T = 120
MOVE = (-2048.0, 4096.0, 300.0)
MAKERS = {
    "ramp": lambda: meshgen.ramp(320, 12, 8.0, 0.05, 1.0, 1.2, 0),
    "torus": lambda: meshgen.torus(64, 32, 2.0, 0.8, 0),
    "tube": lambda: meshgen.tube(48, 40, 0.8, 3.0, 0),
    "moved_ramp": lambda: meshgen.moved(meshgen.ramp(320, 12, 8.0, 0.05, 1.0, 1.2, 0), MOVE),
}
RAMP_NU, RAMP_NV, RAMP_TURNS = 320, 12, 8
# (tiles, most ghosts of a tile) at T = 120, pinned by tests/test_folded_meshes.py
TILINGS = {"ramp": (36, 186), "torus": (19, 74), "tube": (18, 48), "moved_ramp": (36, 199)}


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = Case(MAKERS[name]())
    assert c.weights.min() > 0                                        # no zero-length edge, no coincident vertices
    return c


@functools.lru_cache(maxsize=None)
def tiling(name: str, tile: int = T) -> dict:
    m = case(name).mesh
    return O.tile_batch_tiling(m.xyz, m.faces, m.edges, tile)


@functools.lru_cache(maxsize=None)
def adjacency(name: str):
    """CSR of the vertex neighbours: (ptr, nbr)"""
    m = case(name).mesh
    e = np.asarray(m.edges, np.int64).reshape(-1, 2)
    a = np.concatenate([e[:, 0], e[:, 1]])
    b = np.concatenate([e[:, 1], e[:, 0]])
    order = np.argsort(a, kind="stable")
    ptr = np.zeros(m.V + 1, np.int64)
    np.cumsum(np.bincount(a, minlength=m.V), out=ptr[1:])
    return ptr, b[order]


def ramp_vertex(fu: float, fv: float) -> int:
    """the ramp's vertex at fraction fu along the lane (0 = bottom, 1 = top of the last storey) and fv across it"""
    i = min(RAMP_NU - 1, max(0, int(round(fu * (RAMP_NU - 1)))))
    j = min(RAMP_NV - 1, max(0, int(round(fv * (RAMP_NV - 1)))))
    return j * RAMP_NU + i


def storey_up(v: int) -> int:
    """the vertex one storey above v (same place on the ground, one turn further along the lane)"""
    i, j = v % RAMP_NU, v // RAMP_NU
    step = (RAMP_NU - 1) // RAMP_TURNS
    return j * RAMP_NU + (i + step if i + step < RAMP_NU else i - step)


def full_field(c: Case, seed: int):
    """the whole potential of a wave from `seed` (an infinite offset never cuts it off; the robot vertex does not matter then)"""
    r = c.om.dijkstra(c.weights, c.costs, int(seed), (int(seed) + 1) % c.mesh.V, goal_dist_offset=np.inf)
    assert np.isfinite(r.dist).all()
    return r.dist


@functools.lru_cache(maxsize=None)
def late_ghost_plans(name: str = "ramp", tile: int = T, offsets=(0.0, 0.02, -1e-9)):
    """Plans whose front stops at the goal bound with its only popped vertices near some tile in that tile's LATE ghost slots:
    the wave source is a neighbour of a late ghost outside the tile, the robot stands on the late ghost.  A plan is listed when
      1. no owned vertex of the tile is at or below the bound (the tile is never activated: its owned slots stay +inf),
      2. every ghost of the tile in the slots below 256 is beyond the bound,
      3. none of those ghosts' owner tiles has a vertex at or below the bound (so nothing is exported into those slots either),
      4. the oracle's field holds a finite tentative value on an owned vertex of the tile.
    "At or below the bound" is taken on the full potential against max(goal_dist, dist[robot]) -- below a negative offset the
    engine runs until the robot is reached.  Returns dicts: seed, target, offset, tile, owned (the owned vertices of 4.)."""
    c, Tl = case(name), tiling(name, tile)
    ptr, nbr = adjacency(name)
    vt = Tl["vert_tile"]
    first_late = 256 - tile
    out, seen = [], set()
    fields = {}
    for t in np.flatnonzero(Tl["nh"] > first_late):
        g = Tl["ghost_gid"][Tl["goff"][t]: Tl["goff"][t] + Tl["nh"][t]]
        early, late = g[:first_late], g[first_late:]
        owned = np.flatnonzero(vt == t)
        early_tiles = np.isin(vt, np.unique(vt[early]))
        for tg in late:
            for s in nbr[ptr[tg]: ptr[tg + 1]]:
                if vt[s] == t:
                    continue
                if int(s) not in fields:
                    fields[int(s)] = full_field(c, int(s))
                full = fields[int(s)]
                for off in offsets:
                    if (int(s), int(tg), off, int(t)) in seen:
                        continue
                    seen.add((int(s), int(tg), off, int(t)))
                    bound = max(np.float32(np.float64(full[tg]) + off), full[tg])
                    near = full <= bound
                    if near[owned].any() or near[early].any() or (near & early_tiles).any():
                        continue
                    ref = c.om.dijkstra(c.weights, c.costs, int(s), int(tg), goal_dist_offset=off)
                    tent = owned[np.isfinite(ref.dist[owned])]
                    if ref.code == 0 and tent.size:
                        out.append(dict(seed=int(s), target=int(tg), offset=off, tile=int(t), owned=tent))
    return tuple(out)                                                 # (cached: shared by the tests, left unchanged)


class FoldedWorld(R.World):
    """tests/replan_model.py's World (the cost state two contexts of a replan test hold) on one of these meshes; its key there
    (World.N: R.adjacency, E.classify) is the mesh's name"""

    def __init__(self, name: str):
        super().__init__(name, True, case=case(name))


def ramp_warm_batch(n: int = 72):
    """n plans on the ramp and a patch of blocked vertices on its fourth storey that leaves the outer third of the lane open:
    (seeds, targets, patch ids)"""
    rng = np.random.default_rng(72)
    V = RAMP_NU * RAMP_NV
    s, t = rng.integers(0, V, n), rng.integers(0, V, n)
    t = np.where(t == s, (t + 7) % V, t)
    patch = np.array([j * RAMP_NU + i for j in range(0, 8) for i in range(136, 144)], np.uint32)
    return s.tolist(), t.tolist(), patch


def face_of(c: Case, v: int) -> int:
    """the first face at vertex v"""
    return int(np.flatnonzero((c.mesh.faces == v).any(axis=1))[0])


def face_point(c: Case, f: int) -> np.ndarray:
    """a point inside face f, off its centroid (the faces of a folded mesh are named by id: a position alone is ambiguous
    where two storeys or the two sides of a tube lie over each other)"""
    a, b, d = c.mesh.xyz[c.mesh.faces[f]].astype(np.float64)
    return (0.5 * a + 0.3 * b + 0.2 * d).astype(np.float32)


def torus_opposite(v: int) -> int:
    """the torus vertex half way round the axis from v: two fronts meet on the way"""
    nu = 64
    return (v // nu) * nu + (v % nu + nu // 2) % nu


def plan_pairs(name: str, n: int, seed: int = 5):
    """n (wave source, robot) vertex pairs: the first ones chosen for the mesh (another storey and the whole lane on the ramps,
    opposite sides on the torus, bottom to top on the tube), the rest seeded random"""
    V = case(name).mesh.V
    rng = np.random.default_rng(seed)
    if name in ("ramp", "moved_ramp"):
        a = ramp_vertex(0.31, 0.5)
        first = [(a, storey_up(a)), (ramp_vertex(0.02, 0.2), ramp_vertex(0.98, 0.8)), (ramp_vertex(0.6, 0.0), ramp_vertex(0.6, 1.0))]
    elif name == "torus":
        first = [(v, torus_opposite(v)) for v in (5, 64 * 16 + 40, 64 * 27 + 13)]
    else:
        first = [(3, V - 20), (48 * 20 + 7, 48 * 20 + 31), (V - 1, 0)]
    s = rng.choice(V, n, replace=False)
    t = rng.choice(V, n, replace=False)
    t = np.where(t == s, (t + 1) % V, t)
    for k, (x, y) in enumerate(first[:n]):
        s[k], t[k] = x, y
    return s.astype(np.uint32), t.astype(np.uint32)
