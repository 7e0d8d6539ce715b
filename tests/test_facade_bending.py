"""The C++ facade's bending term (admm::BendingEnergyTerm, create_bending_from_mesh): it compiles
against the C ABI on CPU; on the GPU tests/cpp/facade_bending.cpp's run equals the same scene bound
through the Python binding bit for bit (both drive the identical device path, so any mapping error
shows)."""
import os
import subprocess

import numpy as np
import pytest

import bending_cases as bc
from conftest import REPO
from test_facade import build

SRC = os.path.join(REPO, "tests", "cpp", "facade_bending.cpp")


def test_facade_bending_builds(tmp_path):
    build(str(tmp_path / "facade_bending"), SRC)


@pytest.mark.gpu
def test_facade_bending_matches_binding(tmp_path, pkg, ctx):
    exe, out = str(tmp_path / "facade_bending"), str(tmp_path / "o.bin")
    build(exe, SRC)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:4], np.int32)[0])
    xv = np.frombuffer(raw[4:], np.float64).reshape(2, n, 3)
    sc = bc.grid3_scene()
    assert n == sc.n_nodes and sc.iters == 30 and sc.aa_m == 4 and sc.n_steps == 3
    want, s = pkg.capi.run_scene(ctx, sc)
    s.close()
    assert np.array_equal(xv[0], want[-1]["x"].reshape(-1, 3))
    assert np.array_equal(xv[1], want[-1]["v"].reshape(-1, 3))
    assert np.abs(xv[1]).max() > 0
