"""GPU: the sweep sequence of k_tbv_solve (mesh_navigation_amd/csrc/mnav_tbv.h, mnav_tbv_seq.h).

(a) the sweep routine on its own (mnav_debug_tbv_sweeps_seq) against the numpy emulation of tests/tbv_seq_model.py, bits and sweep
    counts: streams of 30, 31 (a padded last chunk) and 1 chunk per order, 8 waves; every voted-orders prefix of length 1 to 4; an
    item that needs more sweeps than the prefix holds (the rotation behind it, past the sixteen packed entries too); a cap of 3
    on an image that needs more (overrun reported, the image as three sweeps leave it); and the older entry
    (mnav_debug_tbv_sweeps), whose `first_order` still means that order and then the rotation;
(b) whole batches through the C ABI on the C2 terrain recipe at N = 150 (the inputs of the CPU measurement in DESIGN.md 3.1):
    800 and 70 plans, offsets 0.3, inf and -1, the option `tb_sweep_seq` on and off, every plan against the oracle bit for bit;
    and the reason for all this: fewer sweeps per item with the option on (mnav_tb_engine_stats).

The claim itself -- the sequence cannot be seen in the bits -- and the cursors' arithmetic are CPU tests: tests/test_tbv_seq.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import tbv_seq_model as M
from tests.common import terrain_case
from tests.test_gpu_tbv_parity import TBV, assert_engine, assert_fields_equal_oracle

pytestmark = pytest.mark.gpu

WAVES = 8
ARGS = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]


@functools.lru_cache(maxsize=None)
def entries():
    L = capi.load()
    for fn in (L.mnav_debug_tbv_sweeps_seq, L.mnav_debug_tbv_sweeps):
        fn.restype, fn.argtypes = C.c_int, ARGS
    return L.mnav_debug_tbv_sweeps_seq, L.mnav_debug_tbv_sweeps


@functools.lru_cache(maxsize=None)
def stream(nch):
    """(words, orders, images) of a tile with `nch` chunks per order; the images are never written"""
    rng = np.random.default_rng(300 + nch)
    words, orders = M.make_tile_stream(rng, nch)
    img = M.make_images(rng, WAVES, live=64, sources=2)
    img[1, :, 17:] = np.inf                                                    # waves with 17 and with 1 live lane
    img[2, :, 1:] = np.inf
    img.setflags(write=False)
    return words, orders, img


def run_device(fn, words, nch, seq_or_first, cap, img0):
    img = img0.copy()
    res = np.zeros((WAVES, 2), np.uint32)
    ms = C.c_float()
    rc = fn(words.ctypes.data, nch, seq_or_first, cap, 0, 1, WAVES, img.ctypes.data, res.ctypes.data, C.byref(ms))
    assert rc == 0, rc
    return img, res[:, 0].astype(np.int64), res[:, 1].astype(np.int64)


def check(fn, nch, arg, order_of_sweep, cap, tag):
    words, orders, img0 = stream(nch)
    ref = img0.copy()
    want_sweeps, want_over = M.emulate(ref, orders, order_of_sweep, cap)
    img, sweeps, over = run_device(fn, words, nch, arg, cap, img0)
    assert np.array_equal(sweeps, want_sweeps), (tag, sweeps, want_sweeps)
    assert np.array_equal(over, want_over), (tag, over, want_over)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (tag, int((img.view(np.uint32) != ref.view(np.uint32)).sum()))
    return want_sweeps, ref


@pytest.mark.parametrize("nch", [30, 31, 1])
def test_every_voted_prefix_runs_in_its_order_and_leaves_the_same_bits(nch):
    fn, _ = entries()
    fixed = None
    seen = set()
    for prefix, counts in M.prefixes():
        seq = M.pack(M.rule_orders(counts))
        assert [M.seq_at(seq, k) for k in range(len(prefix))] == list(prefix)
        sweeps, ref = check(fn, nch, seq, lambda k, seq=seq: M.seq_at(seq, k), 64, (nch, prefix))
        if fixed is None:
            fixed = ref
        assert np.array_equal(ref.view(np.uint32), fixed.view(np.uint32)), prefix    # one fixed point, whatever the sequence
        seen.add(tuple(sweeps))
    assert len(M.prefixes()) == 64
    if nch > 1:
        assert len(seen) > 1                                                          # (the sweep counts do depend on it)


@pytest.mark.parametrize("nch", [30, 31, 1])
def test_the_rotation_behind_the_prefix_and_the_cap(nch):
    """A long chain against the grain of every order but one needs many sweeps: more than a prefix of 1, 2 and 4 orders, and with
    order 0 never helping more than the sixteen packed entries hold."""
    fn, _ = entries()
    words, orders, img0 = stream(nch)
    for counts in ((5, 0, 0, 0), (0, 3, 0, 9), (1, 2, 3, 4)):
        seq = M.pack(M.rule_orders(counts))
        voted = sum(1 for c in counts if c)
        sweeps, _ = check(fn, nch, seq, lambda k, seq=seq: M.seq_at(seq, k), 64, (nch, counts))
        if nch > 1:
            assert sweeps.max() > voted, (counts, sweeps)                             # the fallback rotation ran
    # a cap of 3 on images that need more: overrun, no fault, the image as three sweeps leave it
    seq = M.pack(M.rule_orders((0, 0, 7, 1)))
    need, _ = check(fn, nch, seq, lambda k: M.seq_at(seq, k), 64, (nch, "uncapped"))
    sweeps, ref = check(fn, nch, seq, lambda k: M.seq_at(seq, k), 3, (nch, "cap 3"))
    if nch > 1:
        assert need.max() > 3
        _, _, over = run_device(fn, words, nch, seq, 3, img0)
        assert list(over) == [1 if s > 3 else 0 for s in need], (over, need)


def test_more_sweeps_than_packed_entries():
    """A stream whose every order is the SAME chain against the grain: one row per sweep, far beyond entry 15 -- the cursors' step
    back by 4 runs on the device, and the cap of 16 T sweeps is not what ends it."""
    fn, _ = entries()
    nch = 30
    words = np.zeros(4 * nch * 64, np.uint32)
    blocks = [(r, [r + 1] + [r] * 5, np.array([0.125] + [np.inf] * 5, np.float32)) for r in range(M.T - 1)] + [(M.T - 1, [M.T - 1] * 6, np.full(6, np.inf, np.float32))]
    orders = []
    for o in range(4):
        for b, (tgt, srcs, w) in enumerate(blocks):
            d = np.zeros(16, np.uint32)
            S = [0x2000 | (64 + x) for x in srcs]
            d[0] = (0xA000 | (64 + tgt)) | (S[0] << 16); d[1] = S[1] | (S[2] << 16); d[2] = S[3] | (S[4] << 16); d[3] = S[5]
            d[8:14] = w.view(np.uint32)
            words[(o * nch + b // 4) * 64 + 4 * np.arange(16) + b % 4] = d
        orders.append((np.array([t for t, _, _ in blocks]), np.array([s for _, s, _ in blocks]), np.stack([w for _, _, w in blocks])))
    img0 = np.full((WAVES, M.T, 64), np.inf, np.float32)
    img0[:, 40, :5] = 0.0                                                      # the value walks from row 40 down to row 0: 40 sweeps + the quiet one
    seq = M.pack(M.rule_orders((0, 2, 0, 1)))
    ref = img0.copy()
    want, over = M.emulate(ref, orders, lambda k: M.seq_at(seq, k), 16 * M.T)
    assert want.min() == 41 and not over.any()
    img, sweeps, ovr = run_device(fn, words, nch, seq, 16 * M.T, img0)
    assert np.array_equal(sweeps, want) and not ovr.any(), (sweeps, ovr)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("first", [0, 1, 2, 3])
def test_the_older_entry_still_means_first_order_then_the_rotation(first):
    _, fn_old = entries()
    for nch in (31, 1):
        check(fn_old, nch, first, lambda k: (first + k) & 3, 64, (nch, "first_order", first))


# ------------------------------------------------------------------------------------------------------------- whole batches
OFFSETS = (0.3, float("inf"), -1.0)
N_SAMPLED = 64


@functools.lru_cache(maxsize=None)
def batch_inputs():
    case = terrain_case(150, 2)
    m = case.mesh
    goals = np.random.default_rng(5).choice(m.V, size=800, replace=False).astype(np.uint32)
    robots = np.full(800, m.vertex_at(0.9, 0.9), np.uint32)
    same = goals == robots
    goals[same] = (goals[same] + 1) % m.V
    return case, goals, robots


@functools.lru_cache(maxsize=None)
def oracle(n, offset):
    """the oracle's result of the first n plans at `offset`, vector maps for the sampled ones: computed once, read by both options"""
    case, goals, robots = batch_inputs()
    sampled = set(int(k) for k in np.random.default_rng(n).permutation(n)[:N_SAMPLED])
    out = []
    for k in range(n):
        ref = case.om.dijkstra(case.weights, case.costs, int(goals[k]), int(robots[k]), goal_dist_offset=offset)
        out.append((ref, case.om.dijkstra_vector_map(ref.pred) if k in sampled else None))
    return out, sorted(sampled)


@pytest.mark.parametrize("n", [800, 70])
def test_batches_equal_the_oracle_with_the_sequence_on_and_off(gpu_ctx_factory, n):
    case, goals, robots = batch_inputs()
    goals, robots = goals[:n], robots[:n]
    ctx = gpu_ctx_factory()
    per_item = {}
    try:
        case.upload(ctx)
        ctx.set_dijkstra_engine("tile_batch")
        ctx.set_option("tb_kernel", 1)
        ctx.set_resident_outputs(True)
        for offset in OFFSETS:
            refs, sampled = oracle(n, offset)
            for on in (1, 0):
                ctx.set_option("tb_sweep_seq", on)
                b = ctx.plan_dijkstra_batch(goals, robots, goal_dist_offset=offset, want_fields=False)
                assert_engine(ctx, TBV)
                st = ctx.tb_engine_stats()
                assert st["items"] > 0 and st["sweeps"] >= st["items"] and st["iterations"] > 0 and st["activations"] >= st["items"], st
                per_item[(offset, on)] = st["sweeps_per_item"]
                for k in range(n):                                             # codes and vertex paths of every plan
                    assert b["codes"][k] == refs[k][0].code, (n, offset, on, k)
                    assert np.array_equal(b["paths"][k], refs[k][0].path), (n, offset, on, k)
                assert_fields_equal_oracle(ctx, b, goals, robots, {k: refs[k] for k in sampled}, ("tb_sweep_seq", on, n, offset))
        for offset in OFFSETS:
            print("n = %d, offset %s: %.3f sweeps per item with tb_sweep_seq = 1, %.3f with 0" % (n, offset, per_item[(offset, 1)], per_item[(offset, 0)]))
        if n == 800:                                                           # (the CPU model: 3.56 against 3.95)
            for offset in OFFSETS:
                assert per_item[(offset, 1)] < per_item[(offset, 0)], (offset, per_item)
    finally:
        ctx.close()
