"""CPU: the sweep sequence of k_tbv_solve (mesh_navigation_amd/csrc/mnav_tbv_seq.h, mnav_tbv.h).

  * the function that builds the sequence from the votes, compiled on the host from the header the kernel includes, against the
    rule as it is stated (tests/tbv_seq_model.py);
  * the claim the kernel rests on: on streams whose four orders hold the same blocks, every sequence that ends on a sweep without
    a change leaves the same bits -- the sequence only decides how many sweeps that takes;
  * the load cursors of the sweep routine, restated in tests/tbv_cursor_main.cpp: built alone with the host sanitizers and run as
    a program (nothing of it is loaded into this process).

The routine itself on the device: tests/test_gpu_tbv_seq.py."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tbv_seq_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mesh_navigation_amd", "csrc")

SHIM = r'''
#include "mnav_tbv_seq.h"
extern "C" unsigned seq_build(unsigned c0, unsigned c1, unsigned c2, unsigned c3) { return tbv_seq::tbv_seq_build(c0, c1, c2, c3); }
extern "C" unsigned seq_rotation(unsigned first) { return tbv_seq::tbv_seq_rotation(first); }
extern "C" unsigned seq_at(unsigned seq, unsigned k) { return tbv_seq::tbv_seq_at(seq, k); }
extern "C" unsigned seq_next_index(unsigned k) { return tbv_seq::tbv_seq_next_index(k); }
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host shim of mnav_tbv_seq.h"
    d = tmp_path_factory.mktemp("tbv_seq_shim")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    lib = d / "libshim.so"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", CSRC, "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    for f in (L.seq_build, L.seq_rotation, L.seq_at, L.seq_next_index):
        f.restype = C.c_uint32
    return L


COUNTS = list(itertools.product((0, 1, 2, 5), repeat=4))


def test_the_sequence_is_the_voted_orders_then_the_rotation(shim):
    for c in COUNTS:
        seq = shim.seq_build(*c)
        got = [(seq >> (2 * k)) & 3 for k in range(16)]
        voted = sorted((o for o in range(4) if c[o] > 0), key=lambda o: (-c[o], o))
        n = len(voted)
        assert got[:n] == voted, (c, got)                                   # exactly the voted orders, by votes, then by index
        assert len(set(got[:n])) == n, (c, got)                             # none of them twice
        prev = voted[-1] if voted else 3
        for k in range(n, 16):                                              # then each entry is the one before it + 1
            assert got[k] == (prev + 1) & 3, (c, k, got)
            prev = got[k]
        assert seq == M.pack(M.rule_orders(c)), (c, hex(seq))
        # past the sixteen entries the rotation goes on (the step back by 4), also by the cursors' own stepping
        rule = list(itertools.islice(M.rule_orders(c), 64))
        idx = 0
        for k in range(64):
            assert shim.seq_at(seq, k) == rule[k] == M.seq_at(seq, k), (c, k)
            assert (seq >> (2 * idx)) & 3 == rule[k], (c, k, idx)
            idx = shim.seq_next_index(idx)
            assert idx <= 15


def test_no_vote_and_one_vote_are_rotations(shim):
    assert [shim.seq_at(shim.seq_build(0, 0, 0, 0), k) for k in range(24)] == [k & 3 for k in range(24)]
    for first in range(4):
        votes = [0] * 4
        votes[first] = 7
        assert shim.seq_rotation(first) == shim.seq_build(*votes)
        assert [shim.seq_at(shim.seq_rotation(first), k) for k in range(24)] == [(first + k) & 3 for k in range(24)]


@pytest.fixture(scope="module")
def tile():
    rng = np.random.default_rng(11)
    words, orders = M.make_tile_stream(rng, 30)
    return rng, orders


@pytest.mark.parametrize("live", [1, 17, 64])
def test_every_sequence_that_ends_on_a_quiet_sweep_leaves_the_same_bits(shim, tile, live):
    rng, orders = tile
    img0 = M.make_images(np.random.default_rng(100 + live), 2, live=live)
    seqs = [list(p) for p in itertools.permutations(range(4))]                 # the 24 fixed permutations, repeated
    seqs += [[o] for o in range(4)]                                            # one order alone, again and again
    seqs += [[int(x) for x in rng.integers(0, 4, 16)] for _ in range(4)]       # and arbitrary ones
    ref, ref_sweeps = None, None
    counts = set()
    for s in seqs:
        img = img0.copy()
        sweeps, over = M.emulate(img, orders, lambda k, s=s: s[k % len(s)], 400)
        assert not over.any(), (s, sweeps)
        # ended on a sweep that changed nothing: one more sweep of EVERY order changes nothing either
        for o in range(4):
            again = img.copy()
            assert not M.sweep(np.ascontiguousarray(again.transpose(1, 0, 2)).reshape(M.T, -1), orders[o]).any(), (s, o)
        if ref is None:
            ref, ref_sweeps = img, sweeps
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), s
        counts.add(tuple(int(x) for x in sweeps))
    assert np.isinf(ref[:, :, live:]).all() and np.isfinite(ref[:, :, :live]).any()
    assert len(counts) > 1, counts                                             # (the sequences do differ -- in the number of sweeps)


def test_the_packed_sequence_runs_the_sweeps_of_the_rule(shim, tile):
    _, orders = tile
    img0 = M.make_images(np.random.default_rng(5), 4, live=64)
    for c in ((0, 0, 0, 0), (3, 0, 0, 0), (0, 0, 9, 0), (1, 0, 40, 5), (2, 2, 0, 2), (1, 2, 3, 4), (0, 5, 0, 5)):
        seq = shim.seq_build(*c)
        a, b = img0.copy(), img0.copy()
        rule = list(itertools.islice(M.rule_orders(c), 400))
        sa, oa = M.emulate(a, orders, lambda k: shim.seq_at(seq, k), 400)
        sb, ob = M.emulate(b, orders, lambda k: rule[k], 400)
        assert np.array_equal(sa, sb) and not oa.any() and not ob.any(), (c, sa, sb)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_load_cursors_stay_inside_the_pass_and_follow_the_sequence(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone cursor program"
    exe = str(tmp_path / "tbv_cursors")
    # the runtimes are linked into the program: it needs nothing preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "tbv_cursor_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr
    assert "every load inside the pass" in run.stdout and "FAILED" not in run.stdout
