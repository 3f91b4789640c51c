"""CPU: the planners' models on meshes that are no height field -- a helicoidal ramp (eight storeys over the same ground), a torus,
a vertical tube and the ramp far from the origin (tests/folded_meshes.py).  The tile-batch engine bisects by coordinates, so on
the ramp a tile is a column through every storey with a rim of ghosts on each: slices of more than 256 slots, tiles that do not fit
the register-resident solve kernel.  tests/test_gpu_folded_meshes.py runs the device on the same meshes; what it relies on is
pinned here: the tilings, and that the plans ending on late ghosts exist."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import folded_meshes as FM
from tests.test_schedule_model import _assert_cvp_fields_equal
from tests.test_tb_model import check

NAMES = sorted(FM.MAKERS)


@pytest.mark.parametrize("name", NAMES)
def test_tilings_of_the_folded_meshes(name):
    """(tiles, most ghosts of a tile) at T = 120, next to TBV_PARITY_MESHES of tests/test_tb_model.py; on the ramps most slices
    are longer than 256 slots (more than 136 ghosts); ramp and torus do not fit k_tbv_solve's 64 ghost rows, the tube does"""
    Tl = FM.tiling(name)
    assert (Tl["tiles"], Tl["max_ghosts"]) == FM.TILINGS[name]
    assert Tl["max_ghosts"] == Tl["nh"].max() and Tl["max_slice"] == Tl["sl"].max() == 120 + ((Tl["max_ghosts"] + 3) & ~3)
    V = FM.case(name).mesh.V
    assert Tl["nv"].sum() == V and (Tl["nv"] <= 120).all() and (np.bincount(Tl["vert_tile"], minlength=Tl["tiles"]) == Tl["nv"]).all()
    assert (Tl["vert_local"] < Tl["nv"][Tl["vert_tile"]]).all()
    for t in range(Tl["tiles"]):                                      # ghosts: other tiles' vertices, ordered by (owner tile, local index)
        g = Tl["ghost_gid"][Tl["goff"][t]: Tl["goff"][t] + Tl["nh"][t]].astype(np.int64)
        key = Tl["vert_tile"][g].astype(np.int64) * 256 + Tl["vert_local"][g]
        assert (Tl["vert_tile"][g] != t).all() and (np.diff(key) > 0).all()
    if name in ("ramp", "moved_ramp"):
        assert int((Tl["nh"] > 136).sum()) >= 8
    if name in ("ramp", "torus"):
        assert Tl["max_ghosts"] > 64
    if name == "tube":
        assert Tl["max_ghosts"] <= 64                                 # the control of the kernel choice test


@pytest.mark.parametrize("tile", [64, 120])
@pytest.mark.parametrize("name", NAMES)
def test_tile_batch_model_on_the_folded_meshes(name, tile):
    c = FM.case(name)
    seeds, targets = FM.plan_pairs(name, 6)
    for offset in (0.3, -0.2):
        r = check(c, seeds, targets, offset=offset, tile=tile, jacobi=1)
        assert r["tiles"] == FM.tiling(name, tile)["tiles"] and r["max_ghosts"] == FM.tiling(name, tile)["max_ghosts"]
    if FM.tiling(name, tile)["max_ghosts"] <= 64 and tile == 120:     # the V layout of the streams where the mesh fits it
        check(c, seeds, targets, offset=0.3, tile=tile, jacobi=3)


def test_late_ghost_plans_exist_on_the_ramp():
    """the coverage condition of the GPU test of the finalize pass's reached test: if a change of the tiling empties this set, this
    test fails instead of that one going blind"""
    P = FM.late_ghost_plans("ramp")
    assert len({(p["seed"], p["target"], p["offset"]) for p in P}) >= 32
    assert len({p["tile"] for p in P}) >= 4
    Tl = FM.tiling("ramp")
    for p in P[:: max(1, len(P) // 40)]:
        t = p["tile"]
        g = Tl["ghost_gid"][Tl["goff"][t]: Tl["goff"][t] + Tl["nh"][t]]
        assert Tl["nh"][t] > 136 and p["target"] in g[136:] and Tl["vert_tile"][p["seed"]] != t
        assert (Tl["vert_tile"][p["owned"]] == t).all() and p["owned"].size > 0
    for off in (0.0, 0.02, -1e-9):
        assert sum(p["offset"] == off for p in P) >= 32, off


def test_the_warm_repair_batch_on_the_ramp_has_repaired_and_kept_plans():
    """what the GPU test of k_tb_warm on long slices relies on: the blocked patch on one storey leaves most of the 72 plans to repair,
    some to keep, and the repaired field of the numpy rule is the oracle's fresh plan"""
    from tests import replan_each_model as E
    from tests import replan_model as R
    from tests.test_gpu_replan_each import model, oracle_all
    seeds, targets, patch = FM.ramp_warm_batch()
    W = FM.FoldedWorld("ramp")
    assert (W.costs[patch] <= R.LIMIT).all()
    old = oracle_all(W, seeds, targets)
    C = W.apply(("costs", patch, 1.5))
    cls = model(W, old, seeds, targets, 0.3, C, targets, 0.3, f=0.0)[0]
    assert len(seeds) >= 70 and int((cls == E.REPAIRED).sum()) >= 20 and int((cls == E.KEPT).sum()) >= 5 and int((cls == E.FRESH).sum()) == 0
    new = oracle_all(W, seeds, targets)
    assert sum(r.code == 0 for r in new) >= 60                        # the open third of the lane: the storeys stay connected
    for p in np.flatnonzero(cls == E.REPAIRED)[:4]:
        code, dist, pred, path, _ = R.replan(W, old[p].dist, seeds[p], targets[p], 0.3, C, targets[p], 0.3)
        assert code == new[p].code and np.array_equal(R.bits(dist), R.bits(new[p].dist)) and np.array_equal(pred, new[p].pred)
        assert np.array_equal(path, new[p].path)


@pytest.mark.parametrize("name", NAMES)
def test_cvp_schedule_model_on_the_folded_meshes(name):
    """six plans per mesh, faces named by id; the first three as in plan_pairs (another storey, the whole lane; the opposite side
    of the torus, where the two fronts meet; the tube from bottom to top)"""
    c = FM.case(name)
    m = c.mesh
    seeds, targets = FM.plan_pairs(name, 6)
    for k, (s, t) in enumerate(zip(seeds, targets)):
        sf, tf = FM.face_of(c, int(s)), FM.face_of(c, int(t))
        sp = FM.face_point(c, sf)
        off = (0.3, 0.3, -0.2, 0.3, np.inf, 0.0)[k]
        ref = c.om.cvp(c.weights, c.costs, c.vn, sp, sf, tf, goal_dist_offset=off)
        sv = m.faces[sf]
        mod = O.schedule_model(1, m.faces, m.edges, c.weights, c.costs, sv, ref.dist[sv], sf, m.faces[tf], offset=off)
        assert ref.code == 0 and mod["verify_bad"] == 0 and mod["verify_flags"] == 0, (name, k)
        _assert_cvp_fields_equal(m, ref, mod)
        if k < 3 and np.isfinite(off) and off > 0:                    # the front had to go all the way: most of the mesh is reached
            assert np.isfinite(ref.dist).sum() > (m.V // 4 if name != "tube" else m.V // 8), (name, k)
