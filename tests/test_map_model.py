"""tests/map_model.py, the model the GPU tests of the resident layer graph compare against (tests/test_gpu_layer_graph.py):
its dependency order and the configurations it refuses, that its update sequence is not vacuous, and -- where the
reference's own code is built (oracle/_ref) -- that full recomputation gives the bits the reference's incremental chain
leaves: notifyChange -> LayerManager::layer_changed -> MeshMap::layerChanged -> updateEdgeWeights(changed), plus
onInputChanged of every dependent layer (layer_manager.cpp:202-263, mesh_map.cpp:454-493)."""
import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from oracle import ref as R
from tests import map_model as M
from tests.common import Case
from tests.map_model import bits

SIZES = [(33, 31), (32, 33), (513, 513), (96, 96)]


def test_dependency_order_puts_inputs_before_users():
    for name in "abc":
        nodes, default, _ = M.graph(name)
        order = M.dependency_order(nodes, default)
        assert sorted(order) == sorted(n["layer"] for n in nodes)
        at = {layer: k for k, layer in enumerate(order)}
        for n in nodes:
            assert all(at[i] < at[n["layer"]] for i in n.get("inputs", ())), (name, order)
    # among ready nodes the declaration order decides
    nodes = [dict(layer=9, kind="max", inputs=[4, 2]), dict(layer=4, kind="input"), dict(layer=2, kind="input"), dict(layer=7, kind="input")]
    assert M.dependency_order(nodes, 9) == [4, 2, 7, 9]


@pytest.mark.parametrize("nodes,default,what", [
    ([dict(layer=64, kind="input")], 64, "slot out of range"),
    ([dict(layer=1, kind="input"), dict(layer=1, kind="input")], 1, "listed twice"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="max", inputs=[0, 5])], 1, "not a node"),
    ([dict(layer=0, kind="input", inputs=[0])], 0, "number of inputs"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="inflation", inputs=[0, 0])], 1, "number of inputs"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="inflation")], 1, "number of inputs"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="avg")], 1, "number of inputs"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="avg", inputs=[0] * 9)], 1, "number of inputs"),
    ([dict(layer=0, kind="input"), dict(layer=1, kind="max", inputs=[0, 2]), dict(layer=2, kind="inflation", inputs=[1])], 1, "cycle"),
    ([dict(layer=1, kind="inflation", inputs=[1])], 1, "cycle"),
    ([dict(layer=0, kind="input")], 3, "default layer"),
    ([], 0, "nodes"),
])
def test_refused_configurations(nodes, default, what):
    with pytest.raises(ValueError, match=what):
        M.dependency_order(nodes, default)


def run_model(name, mesh, nx, ny, mode="avg", factor=1.0):
    case = Case(mesh)
    nodes, default, slots = M.graph(name, mode)
    sc = M.scenario_for(name, nx, ny)
    model = M.MapModel(case.om, case.edge_dist, nodes, default, factor)
    for slot, (c, le) in zip(slots, sc.inputs):
        model.set_input(slot, c, le)
    model.compute()
    return model, sc, slots


@pytest.mark.parametrize("nx,ny", SIZES)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_update_sequence_is_not_vacuous(name, nx, ny):
    """What tests/test_gpu_layer_graph.py asserts of the device's n_changed holds in the model alone: the three
    state-changing updates change some but not all vertices of the default layer, adding and removing flip lethal flags
    and re-run the wave, the cost-only change runs none, and the repeated update changes nothing.  In graph (a) the
    default layer is the inflation of `costs`, a function of its lethal set only: there a cost-only change cannot reach
    the default layer, and D is empty."""
    mesh = M.rect_terrain(nx, ny)
    model, sc, slots = run_model(name, mesh, nx, ny)
    for tag, k, ids, costs, lethal in sc.updates:
        before = model.lethal[slots[k]].copy()
        D = model.update_layer(slots[k], ids, costs, lethal)
        flipped = int((before != model.lethal[slots[k]]).sum())
        if tag in ("add", "remove"):
            assert 0 < D.size < mesh.V and flipped > 0 and model.waves == 1, (tag, D.size, flipped)
        elif tag == "cost":
            assert flipped == 0 and model.waves == 0
            assert (D.size == 0) if name == "a" else (0 < D.size < mesh.V), (tag, D.size)
        elif tag == "nothing":
            assert D.size == 0 and model.waves == 0
        assert np.all(D[1:] > D[:-1])


# ---- against the reference's own chain ---------------------------------------------------------------------------

class RefGraph(R.RefMap):
    """A MeshMap of the reference with graph (a) or (b) of tests/map_model.py as its layer stack, the inputs served by
    the harness's ArrayLayer.  Built through oracle.ref.lib()'s ref_param_* / ref_set_array_layer."""
    NAMES = {0: "costs", 1: "inflation", 2: "second", 3: "combined"}

    def __init__(self, mesh, name, mode, inputs, edge_cost_factor):
        L = R.lib()
        self.xyz, self.faces = R._f32(mesh.xyz).reshape(-1, 3), R._u32(mesh.faces).reshape(-1, 3)
        self.V, self.F = self.xyz.shape[0], self.faces.shape[0]
        self._h = L.ref_new()
        L.ref_set_mesh(self._h, self.V, self.F, R._p(self.xyz), R._p(self.faces))
        ns = b"mesh_map."
        L.ref_param_double(self._h, ns + b"edge_cost_factor", float(edge_cost_factor))
        nodes, default, slots = M.graph(name, mode)
        for slot, (c, le) in zip(slots, inputs):
            nm = self.NAMES[slot].encode()
            L.ref_set_array_layer(self._h, nm, self.V, R._p(R._f32(c)), R._p(R._u8(le)))
            L.ref_param_string(self._h, ns + nm + b".type", b"ref_harness/ArrayLayer")
        order = M.dependency_order(nodes, default)
        L.ref_param_string_array(self._h, ns + b"layers", ",".join(self.NAMES[s] for s in order).encode())
        for n in nodes:
            nm = self.NAMES[n["layer"]].encode()
            if n["kind"] == "inflation":
                L.ref_param_string(self._h, ns + nm + b".type", b"mesh_layers/InflationLayer")
            elif n["kind"] in ("avg", "max"):
                L.ref_param_string(self._h, ns + nm + b".type",
                                   b"mesh_layers/AvgCombinationLayer" if n["kind"] == "avg" else b"mesh_layers/MaxCombinationLayer")
                for i, w in zip(n["inputs"], n["weights"]):
                    L.ref_param_double(self._h, ns + self.NAMES[i].encode() + b".combination_weight", float(w))
            if n.get("inputs"):
                L.ref_param_string_array(self._h, ns + nm + b".inputs", ",".join(self.NAMES[i] for i in n["inputs"]).encode())
        L.ref_param_string(self._h, ns + b"default_layer", self.NAMES[default].encode())
        if not L.ref_read_map(self._h):
            raise RuntimeError("MeshMap::readMap failed: " + L.ref_message(self._h).decode())
        self.E = L.ref_num_edges(self._h)
        self._dij = self._cvp = False


def same_state(rm, model, where):
    assert np.array_equal(bits(rm.vertex_costs()), bits(model.vertex_costs)), where
    assert np.array_equal(bits(rm.edge_weights()), bits(model.edge_weights)), where
    for slot in model.order:
        c, le = rm.layer_costs(RefGraph.NAMES[slot])
        assert np.array_equal(bits(c), bits(model.cost[slot])), (where, slot, int((bits(c) != bits(model.cost[slot])).sum()))
        assert np.array_equal(le, model.lethal[slot]), (where, slot)
    d, vec = rm.inflation_fields("inflation")
    assert np.array_equal(bits(d), bits(model.dist[1])), where
    mv = model.vec[1]
    same = (bits(vec).reshape(-1, 3) == bits(mv).reshape(-1, 3)).all(axis=1) | (np.isnan(vec).any(axis=1) & np.isnan(mv).any(axis=1))
    assert same.all(), (where, int((~same).sum()))


@pytest.mark.skipif(not R.available(), reason="the reference's own code is not built here (oracle/_ref)")
@pytest.mark.parametrize("name,mode,factor", [("a", "avg", 1.0), ("b", "max", 0.0), ("b", "max", 1.0), ("b", "avg", 0.0), ("b", "avg", 1.0)])
def test_full_recomputation_is_the_references_incremental_chain(name, mode, factor):
    """24 x 24 terrain; three ref_update_array_layer calls (one adds lethals, one removes some, one changes costs without
    a flag); after each, vertex_costs(), edge_weights(), layer_costs() of every layer and inflation_fields() of the
    reference equal the model's bits.  The vector field depends on which of the equal-key seeds the heap pops first: the
    oracle runs with the reference's plain heap here (tests/test_ref_pins_oracle.py)."""
    mesh = meshgen.terrain(24, 0.1, 3, amplitude=0.5)
    O.set_heap_ties_by_id(False)
    try:
        model, sc, slots = run_model(name, mesh, 24, 24, mode, factor)
        rm = RefGraph(mesh, name, mode, sc.inputs, factor)
        same_state(rm, model, "readMap")
        for tag, k, ids, costs, lethal in sc.updates[:3]:
            model.update_layer(slots[k], ids, costs, lethal)
            rm.update_array_layer(ids, costs, lethal, name=RefGraph.NAMES[slots[k]])
            same_state(rm, model, tag)
        rm.close()
    finally:
        O.set_heap_ties_by_id(True)
