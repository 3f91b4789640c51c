"""The inputs of tests/test_gpu_engine_knobs.py (the per-plan engines under every band width and launch shape), listed ONCE:
tests/test_engine_knobs_model.py runs every combination listed here through the CPU model of the device schedule, so the GPU
file has no combination without its proof that the input is fair.  Small, seeded, built once per process.

  L  terrain(72, amplitude 0.8), Steepness + Inflation (avg), edge_cost_factor 1: V = 5184, cost-inflated triangles, lethal vertices
  A  terrain(64), uniform random costs below 0.9, edge_cost_factor 3: V = 4096, most faces break the triangle inequality
  H  fan_field(40, 6): the valence-40 hub, more faces than a vertex has item slots in the wide kernel
  X  terrain(96) with costs over the limit and 2 % invalid vertices (tests/test_gpu_planners.py::test_cost_limit_invalid_unreachable): Dijkstra only
  P  X with a closed ring of invalid vertices around a 5 x 5 pocket: a VALID target that no wave reaches (on X itself the random
     blocked vertices enclose no valid one, its unreachable target is an invalid vertex): Dijkstra only
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from mesh_navigation_amd import meshgen
from tests.common import Case, layered_costs

INF = float("inf")
MULTS = (0.05, 0.25, None, 60, 1e6)          # band width in mean edge weights; None: the engine's own default
OFFSETS = (0.3, INF, -1.0)                   # goal_dist_offset
H_MULTS = (0.25, 60, 1e6)
BATCH_MULTS = (0.25, None, 1e6)
BATCH_OFFSETS = (INF, -1.0)
BATCH_N = 34
POCKET = (63, 63, 3)                         # case P: grid column and row of the pocket's centre, half side of the ring
RADII = (0.15, 0.4, 3.0)                    # inflation radius: narrower than an edge ring, the default, wider than most of the map


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    if name == "L":
        base = Case(meshgen.terrain(72, 0.1, 3, amplitude=0.8))
        costs, _ = layered_costs(base, "avg")
        return Case(base.mesh, costs, 1.0)
    if name == "A":
        m = meshgen.terrain(64, 0.1, 5)
        return Case(m, np.random.default_rng(2).uniform(0.0, 0.9, m.V).astype(np.float32), 3.0)
    if name == "H":
        return Case(meshgen.fan_field(40, 6, 1))
    if name == "X":
        mesh = meshgen.terrain(96, 0.1, 13)
        rng = np.random.default_rng(3)
        costs = rng.uniform(0, 1.2, mesh.V).astype(np.float32)
        invalid = (rng.uniform(size=mesh.V) < 0.02).astype(np.uint8)
        s, t = mesh.vertex_at(0.1, 0.1), mesh.vertex_at(0.9, 0.9)
        invalid[[s, t]] = 0
        costs[[s, t]] = 0
        return Case(mesh, costs, 1.0, invalid)
    if name == "P":
        x = case("X")
        N = x.mesh.N
        invalid, costs = x.invalid.copy(), x.costs.copy()
        ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="xy")
        ring = (np.maximum(np.abs(ii - POCKET[0]), np.abs(jj - POCKET[1])) == POCKET[2]).ravel()   # (vertex id = j * N + i)
        invalid[ring] = 1
        inside = POCKET[1] * N + POCKET[0]
        invalid[inside] = 0
        costs[inside] = 0
        return Case(x.mesh, costs, 1.0, invalid)
    raise KeyError(name)


def mean_weight(c: Case) -> float:
    w = float(c.weights.mean())
    assert np.isfinite(w) and w > 0.0
    return w


def band_width(c: Case, mult) -> float:
    """what set_band_width gets: 0 restores the engine's default"""
    return 0.0 if mult is None else mult * mean_weight(c)


def model_delta(c: Case, mult, cvp: bool) -> float:
    """the band width the device runs with (mnav.hip auto_delta, mnav_engines_host.h run_plans): the model's `delta`"""
    if mult is not None:
        return float(np.float32(mult * mean_weight(c)))
    w = c.weights[np.isfinite(c.weights)].astype(np.float64)
    auto = np.float32(3.0 * w.sum() / w.size)
    return float(np.float32(4.0) * auto if cvp else auto)


def max_steps(c: Case) -> int:
    """a context's step cap (mnav_upload_mesh)"""
    return int(400.0 * np.sqrt(float(c.mesh.V)) + 20000.0)


@dataclass(frozen=True)
class CvpPlan:
    sp: tuple
    sf: int
    tf: int

    @property
    def seed_pos(self):
        return np.array(self.sp, np.float32)


def _near_free(c: Case, fi, fj) -> int:
    m = c.mesh
    free = np.where(c.costs < 0.5)[0]
    v = m.vertex_at(fi, fj)
    return int(free[((m.xyz[free, :2] - m.xyz[v, :2]) ** 2).sum(1).argmin()])


@functools.lru_cache(maxsize=None)
def cvp_plans(name: str) -> tuple:
    """the single CVP plans of a case"""
    c = case(name)
    m = c.mesh
    if name == "L":                                                    # tests/test_schedule_model.py::test_cvp_layered_costs_config3
        off = np.array([0.02, 0.01, 0], np.float32)
        pairs = [(m.xyz[_near_free(c, 0.15, 0.15)] + off, m.xyz[_near_free(c, 0.85, 0.85)] + off)]
    elif name == "A":
        off = np.array([0.02, 0.015, 0], np.float32)
        pairs = [(m.xyz[m.vertex_at(0.2, 0.2)] + off, m.xyz[m.vertex_at(0.85, 0.8)] + off)]
    elif name == "H":                                                  # tests/test_gpu_cvp_wide.py::test_wide_kernel_on_irregular_valence_and_adversarial_costs
        out = []
        for sv, tv in ((1 + 5 * 40 + 3, 1 + 5 * 40 + 23), (0, 1 + 5 * 40 + 23)):
            sf = int(np.where((m.faces == sv).any(axis=1))[0][0])
            tf = int(np.where((m.faces == tv).any(axis=1))[0][0])
            sp = m.xyz[m.faces[sf]].mean(axis=0).astype(np.float32)
            out.append(CvpPlan(tuple(float(x) for x in sp), sf, tf))
        return tuple(out)
    else:
        raise KeyError(name)
    out = []
    for sp, tp in pairs:
        sf, _ = c.om.containing_face(sp)
        tf, _ = c.om.containing_face(tp)
        out.append(CvpPlan(tuple(float(x) for x in np.asarray(sp, np.float32)), int(sf), int(tf)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cvp_batch(name: str = "L", n: int = BATCH_N, seed: int = 7):
    """seed positions, seed faces and target faces of a batch: random free vertices moved by a fixed offset
    (tests/test_gpu_cvp_wide.py::_batch); a border vertex lands beside the mesh, so the first plan -- the mesh's last corner -- is one
    without a seed face (INVALID_START) by construction and the rest come as they fall"""
    c = case(name)
    m = c.mesh
    rng = np.random.default_rng(seed)
    verts = rng.choice(np.where(c.costs < 0.5)[0], size=n - 1, replace=False)
    off = np.array([0.02, 0.015, 0.0], np.float32)
    sps = np.stack([m.xyz[m.V - 1] + off] + [m.xyz[v] + off for v in verts]).astype(np.float32)
    sfs = np.array([c.om.containing_face(p)[0] for p in sps], np.uint32)
    assert sfs[0] >= m.F and (sfs < m.F).sum() >= 32                   # (from 32 plans on a batch takes the wide kernel by itself)
    tf, _ = c.om.containing_face(m.xyz[_near_free(c, 0.9, 0.9)] + off)
    return sps, sfs, np.full(n, tf, np.uint32)


@functools.lru_cache(maxsize=None)
def dijkstra_plans(name: str) -> tuple:
    """(seed, target, cost_limit) of the Dijkstra plans of a case; unreachable() tells which of them have a target no wave reaches"""
    c = case(name)
    m = c.mesh
    if name == "L":
        return ((_near_free(c, 0.15, 0.15), _near_free(c, 0.85, 0.85), 1.0),)
    if name == "X":
        s, t = m.vertex_at(0.1, 0.1), m.vertex_at(0.9, 0.9)
        # (the random blocked vertices enclose no valid one: what the wave does not reach on X are its invalid vertices, which no
        #  neighbour relaxes, so one of them is the unreachable target: the wave sweeps the whole map for it)
        full = c.om.dijkstra(c.weights, c.costs, s, t, goal_dist_offset=INF, cost_limit=1.0, invalid=c.invalid)
        cut_off = np.where(~np.isfinite(full.dist))[0]
        assert cut_off.size and c.invalid[cut_off].all()
        return ((s, t, 1.0), (s, int(cut_off[cut_off.size // 2]), 1.0))
    if name == "P":                                                    # a valid vertex behind a closed ring of invalid ones
        t = POCKET[1] * m.N + POCKET[0]
        assert c.invalid[t] == 0
        return ((m.vertex_at(0.1, 0.1), t, 1.0),)
    raise KeyError(name)


def unreachable(name: str, k: int) -> bool:
    return (name, k) in (("X", 1), ("P", 0))


@functools.lru_cache(maxsize=None)
def dijkstra_batch(name: str, n: int, seed: int = 5):
    """seeds and targets of a Dijkstra batch: random valid, passable seeds towards the case's first target"""
    c = case(name)
    ok = (c.costs < 0.5) if c.invalid is None else ((c.costs < 0.5) & (c.invalid == 0))
    free = np.where(ok)[0]
    seeds = np.random.default_rng(seed).choice(free, size=n, replace=False).astype(np.uint32)
    return seeds, np.full(n, dijkstra_plans(name)[0][1], np.uint32)


# ---- the combinations: what the GPU file parametrises over and the model file proves fair
CVP_SINGLE = [(name, k, mult, off) for name in ("L", "A") for k in range(1) for mult in MULTS for off in OFFSETS] \
           + [("H", k, mult, INF) for k in range(2) for mult in H_MULTS]
CVP_BATCH = [("L", mult, off) for mult in BATCH_MULTS for off in BATCH_OFFSETS]
DIJKSTRA_CASES = ("L", "X", "P")
DIJKSTRA_BAND = [(name, k, mult, off) for name, nk in (("L", 1), ("X", 2), ("P", 1)) for k in range(nk) for mult in MULTS for off in OFFSETS]
SHAPE_CASE, SHAPE_MULT, SHAPE_OFFSET = "L", None, 0.3     # the launch-shape tests: one width, one offset (single plans: in the lists above)
CVP_BATCH_SHAPE = [(SHAPE_CASE, SHAPE_MULT, SHAPE_OFFSET)]  # ... and the batch they run


def ident(combo) -> str:
    return "-".join("default" if x is None else str(x) for x in combo)


@functools.lru_cache(maxsize=None)
def lethal_of(name: str = "L"):
    """the inflation wave's input: steepness-lethal vertices of the case's mesh"""
    c = case(name)
    _, lethal = c.om.steepness(c.vn, 0.3)
    assert 0 < lethal.sum() < c.mesh.V // 4
    return lethal
