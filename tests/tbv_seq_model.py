"""The sweep sequence of k_tbv_solve (mesh_navigation_amd/csrc/mnav_tbv_seq.h) restated in Python, and a numpy lockstep emulation of
the sweep routine (mnav_tbv.h, tbv_sweeps) that follows a sequence.  Shared by tests/test_tbv_seq.py (CPU) and
tests/test_gpu_tbv_seq.py (the routine on the device through mnav_debug_tbv_sweeps_seq).

The streams model a TILE: the four orders are four permutations of the same blocks (the same edges), so every order has the same
fixed points -- which is what makes the sequence invisible in the result.  (tools/gpu_tbv_micro.py draws other random edges per
order: good for timing and for one fixed sequence, but its result depends on the sequence.)"""
from __future__ import annotations

import itertools

import numpy as np

T, LANES = 120, 64
INF_BITS = 0x7F800000


# ---- the rule, straight from its statement
def rule_orders(counts):
    """The orders of the sweeps, one after the other, for the votes `counts` (four numbers): the orders with a vote by votes
    descending, ties to the lower order; then the rotation from the last of them; no vote: the rotation from order 0."""
    last = 3
    for o in sorted((o for o in range(4) if counts[o] > 0), key=lambda o: (-counts[o], o)):
        yield o
        last = o
    while True:
        last = (last + 1) & 3
        yield last


def pack(orders) -> int:
    """sixteen 2-bit entries, entry k in bits 2 k + 1 : 2 k"""
    return sum(o << (2 * k) for k, o in enumerate(itertools.islice(orders, 16)))


def seq_at(seq: int, k: int) -> int:
    """the order of sweep k of a packed sequence: an index past 15 steps back by 4"""
    return (seq >> (2 * (k if k < 16 else 12 + (k & 3)))) & 3


def prefixes():
    """every voted-orders prefix of length 1 to 4, as votes that produce it (more votes for the earlier order)"""
    out = []
    for n in range(1, 5):
        for p in itertools.permutations(range(4), n):
            counts = [0, 0, 0, 0]
            for rank, o in enumerate(p):
                counts[o] = 10 - rank
            out.append((p, counts))
    return out


# ---- a tile's sweep stream in the V layout
def make_tile_stream(rng, nch, density=(2, 7)):
    """4 orders x nch chunks x 4 blocks.  min(4 nch, T) relaxing blocks, each with its own target row, in four random orders; the
    rest of every order is do-nothing blocks (the target from itself over +inf weights: what the builder pads with).  Returns
    (stream words, orders) with orders[o] = (tgt [nb], src [nb][6], w [nb][6])."""
    nb, real = 4 * nch, min(4 * nch, T)
    rows = rng.permutation(T)[:real]
    blocks = []
    for tgt in rows:
        n = int(rng.integers(*density))
        srcs = [int(x) for x in rng.choice(rows, n)] + [int(tgt)] * (6 - n)   # (sources among the targets: values travel over several blocks)
        w = np.concatenate([rng.uniform(0.05, 0.3, n).astype(np.float32), np.full(6 - n, np.inf, np.float32)])
        blocks.append((int(tgt), srcs, w))
    pad = (int(rows[0]), [int(rows[0])] * 6, np.full(6, np.inf, np.float32))
    words = np.zeros(4 * nch * 64, np.uint32)
    orders = []
    for o in range(4):
        seq = [blocks[i] for i in rng.permutation(real)] + [pad] * (nb - real)
        for b, (tgt, srcs, w) in enumerate(seq):
            d = np.zeros(16, np.uint32)
            S = [0x2000 | (64 + x) for x in srcs]                              # window rows: 64 ghosts first, owned row r at 64 + r
            d[0] = (0xA000 | (64 + tgt)) | (S[0] << 16); d[1] = S[1] | (S[2] << 16); d[2] = S[3] | (S[4] << 16); d[3] = S[5]
            d[8:14] = w.view(np.uint32)
            base = (o * nch + b // 4) * 64
            words[base + 4 * np.arange(16) + b % 4] = d                       # a chunk stores its four blocks transposed
        orders.append((np.array([t for t, _, _ in seq]), np.array([s for _, s, _ in seq]), np.stack([w for _, _, w in seq])))
    return words, orders


def make_images(rng, waves, live=LANES, inf_share=0.5, sources=1):
    """[waves][T][64] float32: `live` lanes with random values, +inf entries and `sources` zero rows; the other lanes all +inf"""
    img = rng.uniform(0.0, 6.0, (waves, T, LANES)).astype(np.float32)
    img[rng.random(img.shape) < inf_share] = np.inf
    for w in range(waves):
        img[w, rng.integers(0, T, sources), :] = 0.0
    img[:, :, live:] = np.inf
    return img


def sweep(f, order):
    """one Gauss-Seidel sweep of `order` over f [T][L] float32, in place; returns per column whether a row was lowered"""
    tgt, src, w = order
    changed = np.zeros(f.shape[1], bool)
    for b in range(len(tgt)):
        cand = (f[src[b]] + w[b][:, None]).min(axis=0)                     # one float32 add per edge, the minimum over the sources
        low = cand < f[tgt[b]]
        changed |= low
        np.minimum(f[tgt[b]], cand, out=f[tgt[b]])
    return changed


def emulate(img, orders, order_of_sweep, cap):
    """img [waves][T][64] float32, swept in place like the device: every wave for itself, sweep k in order `order_of_sweep(k)`, until
    a sweep lowers nothing in any of its lanes or `cap` sweeps are done.  Returns (sweeps [waves], overrun [waves])."""
    waves = img.shape[0]
    f = np.ascontiguousarray(img.transpose(1, 0, 2)).reshape(T, waves * LANES)
    sweeps, over, running = np.zeros(waves, np.int64), np.zeros(waves, np.int64), np.ones(waves, bool)
    k = 0
    while running.any():
        cols = np.repeat(running, LANES)
        g = f[:, cols]                                                         # (a wave that is done or over is frozen)
        ch = sweep(g, orders[order_of_sweep(k)]).reshape(-1, LANES).any(axis=1)
        f[:, cols] = g
        k += 1
        idx = np.flatnonzero(running)
        sweeps[idx] = k
        over[idx[ch]] = 1 if k >= cap else 0
        running[idx[~ch]] = False
        if k >= cap:
            running[:] = False
    img[...] = f.reshape(T, waves, LANES).transpose(1, 0, 2)
    return sweeps, over
