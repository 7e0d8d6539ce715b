"""The C++ facade's spring term (admm::SpringEnergyTerm, create_springs): it compiles against the C
ABI on CPU; on the GPU tests/cpp/facade_springs.cpp's run equals the same scene bound through the
Python binding bit for bit (both drive the identical device path, so any mapping error -- pairs,
k, rest, mode, a null vertex or rest array -- shows)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from golden_io import scenes
from test_facade import build

SRC = os.path.join(REPO, "tests", "cpp", "facade_springs.cpp")


def facade_scene():
    sc = scenes.spring_net(5, 5, iters=30, aa_m=4, n_steps=3)
    pairs = sc.springs[0][0]
    st, sh = pairs[:40], pairs[40:]
    assert np.array_equal(st, scenes.net_pairs(5, 5, shear=False)) and len(sh) == 32
    sc.springs = [(st, 50.0, None, scenes.SPRING),
                  (sh, 20.0 + np.arange(32.0), np.full(32, 1.1 * (0.25 * np.sqrt(2.0))), scenes.SPRING_TETHER)]
    return sc


def test_facade_springs_builds(tmp_path):
    build(str(tmp_path / "facade_springs"), SRC)


@pytest.mark.gpu
def test_facade_springs_matches_binding(tmp_path, pkg, ctx):
    exe, out = str(tmp_path / "facade_springs"), str(tmp_path / "o.bin")
    build(exe, SRC)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:4], np.int32)[0])
    xv = np.frombuffer(raw[4:], np.float64).reshape(2, n, 3)
    sc = facade_scene()
    assert n == sc.n_nodes and sc.iters == 30 and sc.aa_m == 4 and sc.n_steps == 3
    want, s = pkg.capi.run_scene(ctx, sc)
    s.close()
    assert np.array_equal(xv[0], want[-1]["x"].reshape(-1, 3))
    assert np.array_equal(xv[1], want[-1]["v"].reshape(-1, 3))
    assert np.abs(xv[1]).max() > 0
