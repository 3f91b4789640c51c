"""A model of the resident layer graph (mnav_map_*, include/mnav.h) in NumPy over the oracle's restatements of the
reference's layers: InflationLayer (OracleMesh.inflation), CombinationLayer (oracle.combine) and
MeshMap::computeEdgeWeights (OracleMesh.edge_weights).  It knows nothing incremental: after every update the whole graph
is recomputed, and the change list D is the diff of the default layer before and after.  tests/test_map_model.py pins
"full recomputation == the reference's incremental chain" against the reference's own LayerManager / MeshMap.

Nodes are the dicts of capi.MnavContext.map_configure: layer, kind ("input" | "inflation" | "max" | "avg"), inputs,
weights, and an inflation node's parameters."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

MAX_LAYERS, MAX_INPUTS = 64, 8
KINDS = ("input", "inflation", "max", "avg")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dependency_order(nodes, default_layer):
    """The slots in evaluation order: repeatedly every declared node whose inputs are all placed, in declaration order.
    Raises ValueError for what mnav_map_configure refuses."""
    if not 1 <= len(nodes) <= MAX_LAYERS:
        raise ValueError("1..64 nodes")
    decl = {}
    for n in nodes:
        if not 0 <= n["layer"] < MAX_LAYERS:
            raise ValueError("slot out of range")
        if n["layer"] in decl:
            raise ValueError("a slot is listed twice")
        decl[n["layer"]] = n
        if n["kind"] not in KINDS:
            raise ValueError("unknown node kind")
        k = len(n.get("inputs", ()))
        if not (k == 0 if n["kind"] == "input" else k == 1 if n["kind"] == "inflation" else 1 <= k <= MAX_INPUTS):
            raise ValueError("wrong number of inputs for the node kind")
    for n in nodes:
        if any(i not in decl for i in n.get("inputs", ())):
            raise ValueError("an input is not a node")
    if default_layer not in decl:
        raise ValueError("the default layer is not a node")
    order, placed = [], set()
    while len(order) < len(nodes):
        progress = False
        for n in nodes:
            if n["layer"] in placed or any(i not in placed for i in n.get("inputs", ())):
                continue
            placed.add(n["layer"])
            order.append(n["layer"])
            progress = True
        if not progress:
            raise ValueError("cycle")
    return order


class MapModel:
    def __init__(self, om, edge_dist, nodes, default_layer, edge_cost_factor=0.0, invalid=None):
        self.om, self.edge_dist = om, np.ascontiguousarray(edge_dist, np.float32)
        self.order = dependency_order(nodes, default_layer)
        self.nodes = {n["layer"]: n for n in nodes}
        self.default_layer, self.factor = default_layer, float(edge_cost_factor)
        self.invalid = None if invalid is None else np.ascontiguousarray(invalid, np.uint8)
        self.cost, self.lethal, self.dist, self.vec = {}, {}, {}, {}
        self.vertex_costs = self.edge_weights = None
        self.waves = 0                                                 # inflation nodes whose input's lethal set changed in the last update

    # ---- inputs ----
    def set_input(self, layer, costs, lethal=None):
        assert self.nodes[layer]["kind"] == "input"
        V = self.om.V
        self.cost[layer] = np.array(costs, np.float32).reshape(V)
        self.lethal[layer] = np.zeros(V, np.uint8) if lethal is None else (np.asarray(lethal).reshape(V) != 0).astype(np.uint8)

    def _cfg(self, n):
        d = O.InflationCfg.defaults()
        return O.InflationCfg(n.get("inscribed_radius", d.inscribed_radius), n.get("inflation_radius", d.inflation_radius),
                              n.get("lethal_value", d.lethal_value), n.get("inscribed_value", d.inscribed_value),
                              n.get("cost_scaling_factor", d.cost_scaling_factor))

    # ---- the whole graph ----
    def compute(self):
        for layer in self.order:
            n = self.nodes[layer]
            if n["kind"] == "input":
                assert layer in self.cost, "an input layer is not set"
            elif n["kind"] == "inflation":
                src = n["inputs"][0]
                c, d, v = self.om.inflation(self.lethal[src], self.edge_dist, self._cfg(n), invalid=self.invalid)
                self.cost[layer], self.dist[layer], self.vec[layer] = c, d, v
                self.lethal[layer] = self.lethal[src].copy()
            else:
                ins = n["inputs"]
                self.cost[layer] = O.combine([self.cost[i] for i in ins], n.get("weights", [1.0] * len(ins)), n["kind"])
                self.lethal[layer] = np.bitwise_or.reduce([self.lethal[i] for i in ins]).astype(np.uint8)
        self.vertex_costs = self.cost[self.default_layer].copy()
        self.edge_weights = self.om.edge_weights(self.edge_dist, self.vertex_costs, self.factor)

    def _snapshot(self):
        return {k: v.copy() for k, v in self.cost.items()}, {k: v.copy() for k, v in self.lethal.items()}

    def _recompute(self, source, given_ids, before):
        """after input `source` changed (`before` = the snapshot taken ahead of the change): everything again; returns D"""
        d = self.default_layer
        old_cost, old_lethal = before
        self.compute()
        self.waves = sum(1 for k in self.order if self.nodes[k]["kind"] == "inflation"
                         and not np.array_equal(old_lethal[self.nodes[k]["inputs"][0]], self.lethal[self.nodes[k]["inputs"][0]]))
        if d == source:
            return np.unique(np.asarray(given_ids, np.uint32))
        return np.nonzero((bits(old_cost[d]) != bits(self.cost[d])) | (old_lethal[d] != self.lethal[d]))[0].astype(np.uint32)

    # ---- updates ----
    def update_layer(self, layer, ids, costs, lethal=None):
        """the harness's ArrayLayer::update: in order, so of equal ids the last one counts"""
        assert self.nodes[layer]["kind"] == "input"
        ids = np.asarray(ids, np.uint32).reshape(-1)
        if ids.size and ids.max() >= self.om.V:
            raise ValueError("vertex id out of range")
        costs = np.asarray(costs, np.float32).reshape(-1)
        before = self._snapshot()
        for k, v in enumerate(ids):
            self.cost[layer][v] = costs[k]
            if lethal is not None:
                self.lethal[layer][v] = 1 if lethal[k] else 0
        return self._recompute(layer, ids, before)

    def replace_layer(self, layer, costs, lethal, ids):
        """the caller rewrote an input slot with a writer and reports `ids` (mnav_map_layer_changed, mnav_map_obstacle)"""
        before = self._snapshot()
        self.set_input(layer, costs, lethal)
        return self._recompute(layer, ids, before)


# ---- the scenario both test files run: graphs, inputs and a deterministic update sequence --------------------------

def rect_terrain(nx: int, ny: int, h: float = 0.1, seed: int = 0):
    """an nx x ny jittered grid with smooth heights (vertex id = j * nx + i), as a meshgen mesh"""
    from mesh_navigation_amd import meshgen
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    x = (i + rng.uniform(-0.2, 0.2, i.shape)) * h
    y = (j + rng.uniform(-0.2, 0.2, i.shape)) * h
    z = 0.3 * np.sin(i * 0.21) * np.cos(j * 0.17) + 0.05 * np.sin(i * 1.3 + j * 0.9)
    xyz = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)
    v00 = (np.arange(ny - 1, dtype=np.uint32)[:, None] * np.uint32(nx) + np.arange(nx - 1, dtype=np.uint32)[None, :]).ravel()
    faces = np.stack([v00, v00 + 1, v00 + nx + 1, v00, v00 + nx + 1, v00 + nx], axis=1).reshape(-1, 3).astype(np.uint32)
    return meshgen.from_faces(xyz, faces, N=nx, h=h)


def graph(name: str, mode: str = "avg"):
    """(nodes, default layer, the input slots in the order of Scenario.inputs).  Declared users-first on purpose."""
    if name == "a":                                                  # costs -> inflation (default)
        return [dict(layer=1, kind="inflation", inputs=[0]), dict(layer=0, kind="input")], 1, [0]
    if name == "b":                                                  # combined(costs, inflation(costs), second) (default)
        return [dict(layer=3, kind=mode, inputs=[0, 1, 2], weights=[1.0, 0.5, 0.25]), dict(layer=1, kind="inflation", inputs=[0]),
                dict(layer=0, kind="input"), dict(layer=2, kind="input")], 3, [0, 2]
    if name == "c":                                                  # avg(inflation(max(costs, second)), third) (default)
        return [dict(layer=6, kind="avg", inputs=[1, 4], weights=[0.75, 0.5]), dict(layer=1, kind="inflation", inputs=[5], inflation_radius=0.3,
                                                                                  inscribed_radius=0.15),
                dict(layer=5, kind="max", inputs=[0, 2]), dict(layer=0, kind="input"), dict(layer=2, kind="input"),
                dict(layer=4, kind="input")], 6, [0, 2, 4]
    raise ValueError(name)


class Scenario:
    """Inputs and updates for an nx x ny grid.  inputs[k] = (costs, lethal) of the k-th input slot of graph(); updates =
    (tag, k, ids, costs, lethal or None), k indexing the input slots.  `free_cost_input`: which input takes the cost-only
    update -- one whose costs reach the default layer (in graph (c) the first two inputs only reach it through the
    inflation, that is through their flags)."""

    def __init__(self, nx: int, ny: int, n_inputs: int, free_cost_input: int = 0, seed: int = 5):
        rng = np.random.default_rng(seed)
        V = nx * ny
        vid = lambda i, j: j * nx + i
        self.inputs = []
        for k in range(n_inputs):
            c = rng.uniform(0.0, 0.6, V).astype(np.float32)
            le = np.zeros(V, np.uint8)
            col = (nx // 4, 3 * nx // 4, nx // 2)[k % 3]
            rows = range(ny // 4, 3 * ny // 4) if k == 0 else range(ny // 8, ny // 8 + 3)
            for j in rows:                                             # input 0: a wall; the others: a short stub
                le[vid(col, j)] = 1
                c[vid(col, j)] = 1.0
            self.inputs.append((c, le))
        wall = np.array([vid(nx // 4, j) for j in range(ny // 4, 3 * ny // 4)], np.uint32)
        ci, cj = (5 * nx) // 8, ny // 2
        patch = np.array([vid(i, j) for j in range(cj - 1, cj + 2) for i in range(ci - 1, ci + 2)], np.uint32)
        gone = np.concatenate([patch[:4], wall[: max(2, len(wall) // 3)]]).astype(np.uint32)
        some = (np.arange(37, dtype=np.uint64) * 7919 % V).astype(np.uint32)
        some = np.setdiff1d(np.unique(some), np.concatenate([wall, patch]))   # away from the flags: a cost-only change
        new = rng.uniform(0.0, 0.9, some.size).astype(np.float32)
        p, q = int(patch[8]), int(some[0])
        self.updates = [
            ("add", 0, patch, np.full(patch.size, 1.0, np.float32), np.ones(patch.size, np.uint8)),
            ("remove", 0, gone, np.full(gone.size, 0.2, np.float32), np.zeros(gone.size, np.uint8)),
            ("cost", free_cost_input, some, new, None),
            ("nothing", free_cost_input, some, new, None),
            ("duplicates", 0, np.array([p, q, p, q, p], np.uint32), np.array([0.1, 0.2, 0.3, 0.4, 0.5], np.float32),
             np.array([1, 0, 0, 0, 0], np.uint8)),
        ]


def scenario_for(name: str, nx: int, ny: int) -> Scenario:
    return Scenario(nx, ny, {"a": 1, "b": 2, "c": 3}[name], free_cost_input=2 if name == "c" else 0)
