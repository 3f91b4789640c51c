"""Cost layers on the device: Steepness, the Inflation wave (InflationLayer::waveCostInflation,
inflation_layer.cpp:341-491, replayed on the ordered-wave engine), Combination and the edge weights without a host
copy of a V-sized array -- against the oracle, which tests/test_ref_pins_oracle.py pins to the reference's own
InflationLayer / CombinationLayer / MeshMap code."""
import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from oracle import oracle as O
from tests.common import Case

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def upload(ctx, case):
    ctx.upload_mesh(case.mesh.xyz, case.mesh.faces, case.mesh.edges, case.vn)


@pytest.mark.parametrize("N,seed", [(96, 7), (300, 3), (1000, 3)])      # the last one is BASELINE config 3's mesh, 56 % lethal
def test_inflation_distances_and_costs_are_the_reference_bits(gpu_ctx_factory, N, seed):
    case = Case(meshgen.terrain(N, 0.1, seed))
    steep, lethal = case.om.steepness(case.vn, 0.3)
    cost, dist, _ = case.om.inflation(lethal, case.edge_dist)
    ctx = gpu_ctx_factory()
    upload(ctx, case)
    ctx.layer_upload(0, steep, lethal)                          # the input layer as computed by the oracle: same lethal set
    st = ctx.layer_inflation(1, 0)
    c, le, d = ctx.layer_download(1, distances=True)
    assert np.array_equal(bits(d), bits(dist)), int((bits(d) != bits(dist)).sum())
    assert np.array_equal(bits(c), bits(cost))
    assert np.array_equal(le, lethal)                           # lethal_vertices_ = input->lethals() (:170)
    assert st["bands"] <= 3 and st["steps"] > 0


def test_sparse_sources_wide_radius_invalid_vertices(gpu_ctx_factory):
    rng = np.random.default_rng(0)
    case = Case(meshgen.terrain(128, 0.1, 2))
    m = case.mesh
    lethal = np.zeros(m.V, np.uint8)
    lethal[m.edges[rng.choice(m.E, m.E // 200, replace=False)].ravel()] = 1
    lethal[rng.choice(m.V, m.V // 60, replace=False)] = 1       # plus isolated ones: zero-distance vertices the wave fills around backwards
    invalid = np.zeros(m.V, np.uint8)
    invalid[rng.choice(m.V, m.V // 40, replace=False)] = 1
    ctx = gpu_ctx_factory()
    upload(ctx, case)
    ctx.layer_upload(0, np.zeros(m.V, np.float32), lethal)
    for radius, inv in ((0.4, None), (1.3, None), (1.3, invalid), (0.4, invalid)):
        cfg = O.InflationCfg.defaults()
        cfg.inflation_radius = radius
        cost, dist, _ = case.om.inflation(lethal, case.edge_dist, cfg, invalid=inv)
        ctx.layer_inflation(1, 0, inflation_radius=radius, invalid=inv)
        c, _, d = ctx.layer_download(1, distances=True)
        assert np.array_equal(bits(d), bits(dist)), (radius, inv is not None, int((bits(d) != bits(dist)).sum()))
        assert np.array_equal(bits(c), bits(cost))


def test_c3_cost_stack_stays_on_the_device(gpu_ctx_factory):
    """Steepness -> Inflation -> weighted sum -> edge weights (BASELINE config 3's costs), all resident; then both
    planners on those costs against the oracle on the SAME costs.  Steepness uses the device's acosf, which may
    differ from the host libm's by an ulp, so the stack is compared layer by layer with the device's steepness as
    the common input; the lethal sets must agree exactly on this mesh."""
    case = Case(meshgen.terrain(160, 0.1, 3))
    m = case.mesh
    ctx = gpu_ctx_factory()
    upload(ctx, case)
    ctx.layer_steepness(0, 0.3)
    steep_d, lethal_d = ctx.layer_download(0)
    steep, lethal = case.om.steepness(case.vn, 0.3)
    assert np.array_equal(lethal_d, lethal)
    assert np.max(np.abs(steep_d - steep)) <= 2.5e-7             # acosf: <= 2 ulp near pi/2... 1 ulp of 1.0 = 1.2e-7
    ctx.layer_inflation(1, 0)
    infl_d, _, dist_d = ctx.layer_download(1, distances=True)
    infl, dist, _ = case.om.inflation(lethal, case.edge_dist)
    assert np.array_equal(bits(dist_d), bits(dist)) and np.array_equal(bits(infl_d), bits(infl))
    for mode in ("avg", "max"):
        ctx.combine_layers([0, 1], [1.0, 1.0], mode=mode, edge_cost_factor=1.0)
        vc, w = ctx.download_costs()
        want_vc = O.combine([steep_d, infl_d], [1.0, 1.0], mode)
        want_w = case.om.edge_weights(case.edge_dist, want_vc, 1.0)
        assert np.array_equal(bits(vc), bits(want_vc)) and np.array_equal(bits(w), bits(want_w))
    # planners on the resident costs (max combination left resident)
    free = np.nonzero(want_vc < 0.5)[0]
    s, t = int(free[len(free) // 7]), int(free[-len(free) // 9])
    ref = case.om.dijkstra(want_w, want_vc, s, t)
    out = ctx.plan_dijkstra(s, t)
    assert out.code == ref.code and np.array_equal(bits(out.dist), bits(ref.dist)) and np.array_equal(out.pred, ref.pred)


def test_inflation_vector_field_on_the_device(gpu_ctx_factory):
    """vector_map_ of the inflation layer computed on the device == the sequential oracle, bit for bit (NaN where the
    reference normalises a zero vector), on a terrain and on a punched mesh with boundary / multi-fan vertices."""
    rng = np.random.default_rng(2)
    for mesh in (meshgen.terrain(128, 0.1, 2), meshgen.punched(96, 0.1, 5, drop=0.15)):
        case = Case(mesh)
        _, lethal = case.om.steepness(case.vn, 0.5)
        lethal[mesh.edges[rng.choice(mesh.E, mesh.E // 200, replace=False)].ravel()] = 1
        ctx = gpu_ctx_factory()
        upload(ctx, case)
        ctx.layer_upload(0, np.zeros(mesh.V, np.float32), lethal)
        for radius in (0.4, 1.0):
            cfg = O.InflationCfg.defaults()
            cfg.inflation_radius = radius
            _, dist, vec = case.om.inflation(lethal, case.edge_dist, cfg)
            ctx.layer_inflation(1, 0, inflation_radius=radius)
            _, _, d = ctx.layer_download(1, distances=True)
            assert np.array_equal(bits(d), bits(dist))
            dv, has = ctx.layer_vectors(1)
            a, b = dv.view(np.uint32), np.ascontiguousarray(vec, np.float32).view(np.uint32)
            same = (a == b).all(axis=1) | (np.isnan(dv).any(axis=1) & np.isnan(vec).any(axis=1))
            same |= (has == 0) & (vec == 0).all(axis=1)            # no entry in the reference's map
            assert same.all(), (radius, int((~same).sum()))
            assert has.sum() > lethal.sum() // 2


def test_incremental_combination_equals_the_full_pass(gpu_ctx_factory):
    """CombinationLayer::onInputChanged + layerChanged + updateEdgeWeights(changed): a layer changes on a few hundred
    vertices; recombining only those and re-weighting only the edges around them must give the very arrays the full
    pass gives (both modes, edge_cost_factor 1)."""
    rng = np.random.default_rng(4)
    case = Case(meshgen.terrain(96, 0.1, 9))
    m = case.mesh
    a = rng.uniform(0, 0.6, m.V).astype(np.float32)
    b = rng.uniform(0, 0.6, m.V).astype(np.float32)
    ids = rng.choice(m.V, 300, replace=False).astype(np.uint32)
    b2 = b.copy()
    b2[ids] = rng.uniform(0, 1.4, ids.size).astype(np.float32)
    for mode in ("max", "avg"):
        ctx = gpu_ctx_factory()
        upload(ctx, case)
        ctx.layer_upload(0, a); ctx.layer_upload(1, b)
        ctx.combine_layers([0, 1], [1.0, 0.5], mode=mode, edge_cost_factor=1.0)
        ctx.layer_upload(1, b2)                                      # the layer changed (here: re-uploaded)
        ctx.combine_layers_update([0, 1], ids, [1.0, 0.5], mode=mode)
        vc, w = ctx.download_costs()
        ctx.combine_layers([0, 1], [1.0, 0.5], mode=mode, edge_cost_factor=1.0)
        vc_full, w_full = ctx.download_costs()
        assert np.array_equal(bits(vc), bits(vc_full)) and np.array_equal(bits(w), bits(w_full))
        want = O.combine([a, b2], [1.0, 0.5], mode)
        assert np.array_equal(bits(vc), bits(want))


def _sparse_lethal_case(i):
    """the generator of tools/gpu_infl_fuzz.py (round 5), configurations by index"""
    rng = np.random.default_rng(5000 + i)
    N = int(rng.choice([64, 128, 200])); seed = int(rng.integers(1000)); amp = float(rng.choice([0.3, 0.8]))
    kind = int(rng.integers(3)); a = float(rng.choice([0.3, 0.5])); b = int(rng.choice([100, 400])); c = int(rng.choice([30, 300]))
    use_inv = bool(rng.random() < 0.5); radius = float(rng.choice([0.25, 0.4, 0.9, 1.3]))
    case = Case(meshgen.terrain(N, 0.1, seed, amplitude=amp))
    m = case.mesh
    lethal = np.zeros(m.V, np.uint8)
    if kind == 0:
        _, lethal = case.om.steepness(case.vn, a)
    elif kind == 1:
        lethal[m.edges[rng.choice(m.E, max(1, m.E // b), replace=False)].ravel()] = 1
        lethal[rng.choice(m.V, max(1, m.V // 80), replace=False)] = 1
    else:
        lethal[rng.choice(m.V, max(1, m.V // c), replace=False)] = 1
    inv = None
    if use_inv:
        inv = np.zeros(m.V, np.uint8)
        inv[rng.choice(m.V, m.V // 40, replace=False)] = 1
    return case, lethal, inv, radius


@pytest.mark.parametrize("i", [129, 40, 16, 62, 67, 84, 745, 1211, 5438, 7515])
def test_isolated_lethal_vertices_with_tied_pop_times_settle(gpu_ctx_factory, i):
    """Isolated lethal vertices on the regular grid make vertices of EXACTLY the same pop time, and cascades below them whose members
    support each other with provisional keys: such a band kept flipping under the concurrent in-place evaluation until the step cap
    (16 of 209 random maps of the round-5 soak: INTERNAL_ERROR; with a serial band 2-3 %, with a serial band from a reset state
    0.5 % -- configurations 62, 67, 84 and 745, 1211, 5438 of tools/gpu_infl_fuzz.py are what each stage left).  Since round 6 a
    narrow band that does not settle goes through the exact band routine (mnav_eval.h exact_*, k_exact_band: one pop at a time, the
    reference's own procedure; reproduced and fixed on the CPU model first, tests/test_inflation_model.py).  Distances and costs are
    the reference's bits."""
    case, lethal, inv, radius = _sparse_lethal_case(i)
    cfg = O.InflationCfg.defaults()
    cfg.inflation_radius = radius
    cost, dist, _ = case.om.inflation(lethal, case.edge_dist, cfg, invalid=inv)
    ctx = gpu_ctx_factory()
    upload(ctx, case)
    ctx.layer_upload(0, np.zeros(case.mesh.V, np.float32), lethal)
    st = ctx.layer_inflation(1, 0, inflation_radius=radius, invalid=inv)
    c, _, d = ctx.layer_download(1, distances=True)
    assert np.array_equal(bits(d), bits(dist)), int((bits(d) != bits(dist)).sum())
    assert np.array_equal(bits(c), bits(cost))
    assert st["steps"] < 20000                                         # (a band that goes through the exact band routine idles through the rest of its chunk of steps)


@pytest.mark.parametrize("writer", ["upload", "steepness"])
def test_a_plain_layer_written_over_an_inflation_layer_drops_its_wave_state(gpu_ctx_factory, writer):
    """A slot that held an inflation layer and is then overwritten by mnav_layer_upload / mnav_layer_steepness holds a plain
    layer: its costs and flags are the new ones bit for bit, and the old wave's distances and vector field are gone -- they
    cannot be downloaded, and the back-tracking does not steer on them."""
    rng = np.random.default_rng(11)
    mesh = meshgen.terrain(44, 0.1, 12, amplitude=0.3)
    N = mesh.N
    lethal = np.zeros(mesh.V, np.uint8)
    i, j = np.meshgrid(np.arange(N), np.arange(N))
    lethal[(((j == 18) | (j == 25)) & (i > 3) & (i < N - 4)).ravel()] = 1            # a corridor between two lethal walls
    case = Case(mesh)
    goal = mesh.xyz[21 * N + 6] + np.array([0.02, 0.03, 0.0], np.float32)
    robot = mesh.xyz[22 * N + N - 8] + np.array([0.03, 0.01, 0.0], np.float32)
    sf, _ = case.om.containing_face(goal)
    tf, _ = case.om.containing_face(robot)
    ctx = gpu_ctx_factory()
    upload(ctx, case)
    ctx.layer_upload(0, np.zeros(mesh.V, np.float32), lethal)
    ctx.layer_inflation(1, 0)
    ctx.combine_layers([1], [1.0], mode="max", edge_cost_factor=1.0)
    ctx.set_resident_outputs(True)
    assert ctx.plan_cvp(goal, sf, tf, want_fields=False, want_vecmap=False).code == 0
    # the inflation layer: distances, a vector field, and the walk takes it
    ctx.layer_download(1, distances=True)
    ctx.layer_vectors(1)
    assert ctx.backtrack_cvp(goal, sf, robot, tf, step_width=0.2, inflation_layer=1)[0] == 1
    if writer == "upload":
        want_c = rng.uniform(0, 1.4, mesh.V).astype(np.float32)
        want_l = (rng.random(mesh.V) < 0.1).astype(np.uint8)
        ctx.layer_upload(1, want_c, want_l)
    else:
        ctx.layer_steepness(2, 0.3)                              # the device's own steepness, in a slot that never held a wave
        want_c, want_l = ctx.layer_download(2)
        ctx.layer_steepness(1, 0.3)
    c, le = ctx.layer_download(1)
    assert np.array_equal(bits(c), bits(want_c)) and np.array_equal(le, want_l)
    with pytest.raises(RuntimeError, match="this layer keeps no distances"):
        ctx.layer_download(1, distances=True)
    with pytest.raises(RuntimeError, match="this layer has no vector field"):
        ctx.layer_vectors(1)
    with pytest.raises(RuntimeError, match="back-tracking: not a resident inflation layer with a vector field"):
        ctx.backtrack_cvp(goal, sf, robot, tf, step_width=0.2, inflation_layer=1)
    assert ctx.backtrack_cvp(goal, sf, robot, tf, step_width=0.2)[0] == 1           # the plan's own field is untouched
