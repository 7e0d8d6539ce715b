"""The C++ facade's tie term (admm::TieEnergyTerm, create_ties): it compiles against the C ABI on CPU;
on the GPU tests/cpp/facade_ties.cpp's run equals the same scene bound through the Python binding
bit for bit (both drive the identical device path, so any mapping error -- nodes, weights, na / nb,
k, rest, mode, a null vertex or rest array -- shows)."""
import os
import subprocess

import numpy as np
import pytest

import tie_cases as tc
from conftest import REPO
from golden_io import scenes
from test_facade import build

SRC = os.path.join(REPO, "tests", "cpp", "facade_ties.cpp")


def facade_scene():
    sc = tc.pendants(scenes.SPRING_TETHER)
    sc.pin_vel = np.zeros((3, 3))
    ia, wa, ib, wb, _, _, mode = sc.ties[0]
    sc.ties = [(ia, wa, ib, wb, 50.0 + np.arange(3.0), np.full(3, 0.3), mode),
               (np.array([[0, 1]], np.int32), np.array([[0.25, 0.75]]), np.array([[4, 5]], np.int32), np.array([[0.5, 0.5]]), 20.0, None,
                scenes.SPRING)]
    return sc


def test_facade_ties_builds(tmp_path):
    build(str(tmp_path / "facade_ties"), SRC)


@pytest.mark.gpu
def test_facade_ties_matches_binding(tmp_path, pkg, ctx):
    exe, out = str(tmp_path / "facade_ties"), str(tmp_path / "o.bin")
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
