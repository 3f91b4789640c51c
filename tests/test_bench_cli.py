"""CPU: bench.py's command line and its --dump-outputs writer (no GPU: the context is a stand-in that hands out
seeded arrays the way MnavContext.download_output does)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Ctx:
    def __init__(self, V):
        self.V = V

    def download_output(self, what, slot):
        rng = np.random.default_rng(slot)
        if what == "vecmap":
            return rng.random((self.V, 3), dtype=np.float32)
        if what == "pred":
            p = rng.integers(0, self.V, self.V).astype(np.uint32)
            p[::7] = 0xFFFFFFFF                                          # unreached vertices
            return p
        d = rng.random(self.V, dtype=np.float32)
        d[::5] = np.inf                                                  # beyond the plan's cut-off
        return d


def _result(B, V):
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 200, B).astype(np.uint32)
    paths = [rng.integers(0, V, int(n)).astype(np.uint32) for n in lens]
    return {"codes": np.zeros(B, np.uint32), "path_len": lens, "paths": paths}


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_are_float_arrays_within_the_limit_and_repeatable(tmp_path):
    B, V = 2000, 300_000
    ctx, r = _Ctx(V), _result(B, V)
    bench.dump_outputs(str(tmp_path / "a"), ctx, r, V)
    bench.dump_outputs(str(tmp_path / "b"), ctx, r, V)
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert a.keys() == b.keys() >= {"codes", "path_len", "sample_plans", "sample_paths", "dist", "reached", "pred", "vecmap"}
    assert all(a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all() for k in a)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_LIMIT
    plans = a["sample_plans"].astype(np.int64)
    assert np.array_equal(a["sample_paths"], np.concatenate([r["paths"][k] for k in plans]).astype(np.float32))
    verts = a["field_vertices"].astype(np.int64)
    assert np.array_equal(a["pred"][0], ctx.download_output("pred", int(plans[0]))[verts].astype(np.float64))
    d = ctx.download_output("dist", int(plans[0]))[verts]
    assert np.array_equal(a["reached"][0] == 1, np.isfinite(d)) and (a["reached"][0] == 0).any()
    assert np.array_equal(a["dist"][0], np.where(np.isfinite(d), d, -1))


def test_steps_must_be_at_least_one():
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert cp.returncode == 2 and "--steps" in cp.stderr
