"""Worlds for tests/test_gpu_context_lifetime.py: the world of tests/test_gpu_fleet.py (random costs with some above the
limit, a 2 % invalid mask, computed weights, vertex normals, the oracle, plans among the usable vertices, a robot set), but
over ANY mesh -- and with everything the CPU side of a stop needs computed once and kept: the oracle's plans, the robots, the
inputs of the layers, the follower's robots and the vector maps its model reads.

The four meshes make every size-dependent quantity of a context grow and shrink, and none has a vertex count that is a
multiple of 64:

  S  terrain(23): 529 vertices, 8 full tiles of 64 and a ninth of 17
  L  punched(43) with a cut column: 1849 vertices, holes, two components and face-less vertices; other F / V and E / V than S
  T  the two triangles of test_two_triangle_mesh_closed_form: V = 4, F = 2, one tile
  H  hub_terrain(25) with one hub of valence 40: 625 vertices, max_ne / max_nh and both LDS sizes change while V stays small
"""
from __future__ import annotations

import functools

import numpy as np

from mesh_navigation_amd import meshgen
from tests import fleet_model as FM
from tests import follow_model as FOL
from tests.common import Case

LIMIT, OFFSET = 0.8, 0.3                          # as tests/test_gpu_fleet.py
NONE = FM.NONE
PLANS_AND_ROBOTS = {"S": (3, 70), "L": (9, 700), "T": (1, 2), "H": (5, 130)}
HUB = (12, 12, 5)                                # one hub of valence 8 * 5 in the middle of the 25 x 25 grid


def two_triangles():
    xyz = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0]], np.float32)
    return meshgen.from_faces(xyz, np.array([[0, 1, 2], [1, 3, 2]], np.uint32))


MESHES = {
    "S": lambda: meshgen.terrain(23, 0.1, 6),
    "L": lambda: meshgen.punched(43, 0.1, 5, drop=0.30, cut_column=27),
    "T": two_triangles,
    "H": lambda: meshgen.hub_terrain(25, [HUB], 0.1, 3),
}


def fleet_robots(W, fields, n, seed):
    """robots() of tests/test_gpu_fleet.py (imported late: that module is a test file)"""
    from tests.test_gpu_fleet import robots
    return robots(W, fields, n, seed)


class LifetimeWorld:
    """One mesh with its map, plans and robots.  Reads like tests.test_gpu_fleet.World (mesh, V, costs, invalid, case, om,
    weights, seeds, targets, fresh(), fields(), change_costs()), so the check helpers of the fleet tests take it as it is.

    Plans (n_plans of them): plans that succeed, then -- from three plans on -- one towards an invalid vertex (it runs and
    finds no path: its cut is +inf), one whose seed is its target and, from six plans on, one with a target id out of range."""

    def __init__(self, name: str, tile_size: int = 64, seed: int = 17):
        self.name, self.tile_size = name, tile_size
        self.mesh = MESHES[name]()
        V = self.V = self.mesh.V
        self.n_plans, self.n_robots = PLANS_AND_ROBOTS[name]
        rng = np.random.default_rng(seed)
        self.deg = np.bincount(self.mesh.edges.ravel(), minlength=V)
        tiny = V < 16
        self.costs = (rng.random(V) * (0.5 if tiny else 1.0)).astype(np.float32)          # (the smallest mesh stays passable)
        self.invalid = np.zeros(V, np.uint8) if tiny else (rng.random(V) < 0.02).astype(np.uint8)
        self.costs0 = self.costs
        self.case = Case(self.mesh, self.costs, 1.0, self.invalid)
        # a face-less vertex has no normal (NaN): tests/nbhd_model.py sums normals in fixed point and is not defined for those,
        # so such a vertex gets +z -- in the model's arrays and on the device alike (the normals are the caller's data)
        self.case.vn = np.where(np.isfinite(self.case.vn).all(axis=1, keepdims=True), self.case.vn, np.float32([0.0, 0.0, 1.0])).astype(np.float32)
        self.om = self.case.om
        self.weights = self.case.weights
        self.state = "base"                                                                # names the cost changes applied: the key of fresh()
        self._fresh = {}
        self.ok = np.flatnonzero((self.costs <= LIMIT) & (self.invalid == 0) & (self.deg > 0))
        self._pick_plans(rng)
        self.running = np.arange(self.n_run + self.n_nopath)                                # the plans that reach the device
        self._robots = None

    # -- the map ---------------------------------------------------------------------------------------------------------
    def upload(self, ctx):
        ctx.set_option("tile_size", self.tile_size)                                        # (read at upload_mesh)
        ctx.upload_mesh(self.mesh.xyz, self.mesh.faces, self.mesh.edges, self.case.vn)
        self.upload_costs(ctx)

    def upload_costs(self, ctx):
        ctx.compute_edge_weights(self.costs, self.case.edge_dist, 1.0, self.invalid)

    def change_costs(self, ctx, ids, value, state):
        """mnav_update_costs on the context and on the model's state, which is called `state` from here on"""
        self.costs = self.costs.copy()
        self.costs[ids] = value
        self.weights = self.om.edge_weights(self.case.edge_dist, self.costs, 1.0)
        self.state = state
        ctx.update_costs(np.asarray(ids, np.uint32), np.full(len(ids), value, np.float32))

    def restore_costs(self):
        self.costs, self.weights, self.state = self.costs0, self.case.weights, "base"

    # -- plans -----------------------------------------------------------------------------------------------------------
    def fresh(self, seed, v, offset=OFFSET):
        """the oracle's plan from seed to v on the present costs, computed once"""
        key = (self.state, int(seed), int(v), offset)
        if key not in self._fresh:
            self._fresh[key] = self.om.dijkstra(self.weights, self.costs, int(seed), int(v), offset, LIMIT, self.invalid)
        return self._fresh[key]

    def _pick_plans(self, rng):
        P, V, ok = self.n_plans, self.V, self.ok
        self.n_nopath = 1 if P >= 3 else 0
        self.n_rejected = 0 if P < 3 else 1 if P < 6 else 2
        self.n_run = P - self.n_nopath - self.n_rejected
        seeds, targets = [], []
        for _ in range(400):
            if len(seeds) == self.n_run:
                break
            s, t = (int(x) for x in rng.choice(ok, 2, replace=False))
            if s not in seeds and self.fresh(s, t).code == FM.SUCCESS:
                seeds.append(s)
                targets.append(t)
        assert len(seeds) == self.n_run, (self.name, len(seeds))
        if self.n_nopath:
            walled = np.flatnonzero((self.invalid == 1) & (self.deg > 0))
            assert walled.size, self.name
            seeds.append(targets[0])
            targets.append(int(walled[0]))
            assert self.fresh(seeds[-1], targets[-1]).code == FM.NO_PATH_FOUND, self.name
        if self.n_rejected >= 1:
            same = int(ok[len(ok) // 2])
            seeds.append(same)
            targets.append(same)
        if self.n_rejected >= 2:
            seeds.append(int(ok[len(ok) // 3]))
            targets.append(V + 5)
        self.seeds, self.targets = np.array(seeds, np.uint32), np.array(targets, np.uint32)

    def fields(self, targets=None, offset=OFFSET, plans=None):
        """the plans of the batch as the model sees them (the oracle's fields of the plans that run); plans: a subset"""
        t = self.targets if targets is None else targets
        out = []
        for k in (range(len(self.seeds)) if plans is None else plans):
            s, g = int(self.seeds[k]), int(t[k])
            code = FM.plan_code(s, g, self.V)
            if code != FM.SUCCESS or s == g:
                out.append(FM.Field(None, None, s, g, offset, code))
            else:
                r = self.fresh(s, g, offset)
                out.append(FM.Field(r.dist, r.pred, s, g, offset))
        return out

    def plan_codes(self):
        """the code the plan call gives every plan of the batch"""
        return np.array([f.code if f.dist is None else self.fresh(f.seed, f.target).code for f in self.fields()], np.uint32)

    # -- robots ----------------------------------------------------------------------------------------------------------
    def robots(self):
        """(slots, vertices) of the world's robot set over fields(): tests.test_gpu_fleet.robots, computed once"""
        if self._robots is None:
            fields, n = self.fields(), self.n_robots
            slots, vtx = fleet_robots(self, fields, n, 5)
            # the second half of robots() stands on random vertices, many of them beyond a small field: most of those move
            # to a vertex their plan's wave settled, so that at least 40 % of the fleet adds to the traffic
            rng = np.random.default_rng(6)
            for i in range(n // 2, n if n >= 64 else 0):
                f = fields[int(slots[i])]
                if f.dist is not None and rng.random() < 0.8:
                    inside = np.flatnonzero(f.dist < FM.cut_of(f.dist, f.target, f.offset))
                    if inside.size:
                        vtx[i] = rng.choice(inside)
            self._robots = (slots, vtx)
        return self._robots

    @functools.cached_property
    def follow_model(self):
        return FOL.Model(self.mesh, self.om, self.costs0)

    @functools.cached_property
    def follow_robots(self):
        """n_robots robots of every query family of tests/follow_model.py over the running plans (on a mesh of a handful
        of faces: robots inside the faces, one with its face and one without), with a goal per robot: the mesh's middle,
        heading +x"""
        m, n, n_slots = self.follow_model, self.n_robots, len(self.running)
        if m.F < 16:
            rng = np.random.default_rng(3)
            f = np.arange(n) % m.F
            robots = dict(pos=FOL.face_points(m, f, rng).astype(np.float32), dir=np.tile(np.array([1, 0, 0], np.float32), (n, 1)),
                          up=np.tile(np.array([0, 0, 1], np.float32), (n, 1)), face_in=np.where(np.arange(n) % 2 == 0, f, NONE).astype(np.uint32),
                          slot=(np.arange(n) % n_slots).astype(np.uint32), seed_face=None)
        else:
            full, _ = FOL.make_robots(m, n_slots, np.full(n_slots, NONE, np.uint32), 700, per_family=-(-n // len(FOL.FAMILIES)))
            keep = np.sort(np.random.default_rng(4).permutation(full["pos"].shape[0])[:n])
            robots = {k: v[keep] for k, v in full.items()}
            robots["slot"] = (np.arange(n) % n_slots).astype(np.uint32)
            robots["seed_face"] = None
        cen = m.xyz[m.faces].astype(np.float64).mean(axis=1)
        mid = cen[int(np.argmin(np.linalg.norm(cen - np.nanmean(cen, axis=0), axis=1)))].astype(np.float32)
        return robots, (np.tile(mid, (n, 1)), np.tile(np.array([1, 0, 0], np.float32), (n, 1)))

    # -- layers ----------------------------------------------------------------------------------------------------------
    @functools.cached_property
    def layer_inputs(self):
        """lethal flags and costs of the uploaded layers, the two obstacle clouds (300 points hovering over a few random vertices;
        the second one the first half of the first, shifted) and the graph's one update of its first input"""
        rng = np.random.default_rng(23)
        V, xyz = self.V, self.mesh.xyz
        lethal = (rng.random(V) < 0.03).astype(np.uint8)
        if not lethal.any():
            lethal[V - 1] = 1
        under = rng.choice(V, max(2, V // 20), replace=False)                               # (a cloud over a twentieth of the mesh: most of it stays free)
        cloud = (xyz[rng.choice(under, 300)] + rng.uniform(-0.03, 0.03, (300, 3)).astype(np.float32) + np.float32([0.0, 0.0, 0.5])).astype(np.float32)
        cloud2 = (cloud[:150] + np.float32([0.04, 0.03, 0.0])).astype(np.float32)
        third = rng.uniform(0.0, 0.6, V).astype(np.float32)
        ids = rng.choice(V, min(6, V), replace=False).astype(np.uint32)
        upd_cost = rng.uniform(0.0, 0.9, ids.size).astype(np.float32)
        upd_lethal = (np.arange(ids.size) % 2 == 0).astype(np.uint8)
        return dict(lethal=lethal, cloud=cloud, cloud2=cloud2, third=third, ids=ids, upd_cost=upd_cost, upd_lethal=upd_lethal)

    # -- the replans -----------------------------------------------------------------------------------------------------
    @functools.cached_property
    def cost_changes(self):
        """three cost changes of 5 + 3 + 2 vertices (as many as the mesh has beside the seeds) among the vertices the first
        running plan's wave settled below its cut, so that a replan has something to rewind"""
        r = self.fresh(self.seeds[0], self.targets[0])
        cut = FM.cut_of(r.dist, int(self.targets[0]), OFFSET)
        inside = np.flatnonzero(np.isfinite(r.dist) & (r.dist < cut) & ~np.isin(np.arange(self.V), self.seeds))
        pick = np.random.default_rng(29).permutation(inside)[:10].astype(np.uint32)
        return [pick[:5], pick[5:8], pick[8:10]]


@functools.lru_cache(maxsize=None)
def world(name: str, tile_size: int = 64) -> LifetimeWorld:
    return LifetimeWorld(name, tile_size)


def input_conditions(W: LifetimeWorld) -> dict:
    """What keeps a stop from passing vacuously, from the models and the oracle alone (no device): the counts the tests
    assert and the summary lists."""
    from tests import obstacle_model as OM
    from tests import timed_traffic_model as XM
    from tests import traffic_model as TM
    from tests.test_timed_traffic_model import timing
    fields = W.fields()
    codes = W.plan_codes()
    sl, vt = W.robots()
    run = FM.run(fields, W.V, sl, vt)
    tr = TM.traffic(TM.Counts(W.V), fields, sl, vt)
    over = {}
    for B in (5, 70):
        depart, pace, key, tau = timing(len(sl), fields, B, 11 * len(sl) + B)
        over[B] = XM.timed(XM.Cells(W.V), fields, sl, vt, None, depart, pace, key, B, tau, 1, False, run=run)["over_cells"]
    L = W.layer_inputs
    obs = OM.obstacle_layer(W.mesh.xyz, W.mesh.faces, L["cloud"])
    obs2 = OM.obstacle_layer(W.mesh.xyz, W.mesh.faces, L["cloud2"], old_lethal=obs["lethal"])
    r = W.fresh(W.seeds[0], W.targets[0])
    first = W.cost_changes[0]
    return dict(plans=len(codes), success=int(((codes == FM.SUCCESS) & (W.seeds != W.targets)).sum()),
                rejected=int(sum(f.dist is None for f in fields)), robots=len(sl), contributing=tr["contributing"],
                beyond_field=run["counts"][1], no_path=run["counts"][2], over_cells=over,
                obstacle_lethal=int(obs["lethal"].sum()), graph_changed=int(obs2["changed"].size),
                rewound=int(np.isfinite(r.dist[first]).sum()))
