"""CPU tests of the kinematic mesh obstacle: the poses are rotations, the numpy restatement of the
device transform (tests/kinematic_cases.py) has the right direction -- the obstacle-frame oracle
mapped back agrees with an oracle on the world-frame mesh -- the host's pose validation
(csrc/mesh_obstacle.hpp) in a stand-alone program, and the scene layer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kinematic_cases as kc
import mesh_obs_cases as mc
from conftest import REPO
from golden_io import scenes

CSRC = os.path.join(REPO, "aa-admm_amd", "csrc")


@pytest.mark.parametrize("pose", list(kc.POSES))
def test_poses_are_rotations(pose):
    R, t = kc.POSES[pose]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
    Q = np.random.default_rng(3).normal(size=(50, 3))
    assert np.abs(kc.to_world(R, t, kc.to_local(R, t, Q)) - Q).max() <= 1e-14
    assert np.abs(kc.to_world(R, t, Q) - (Q @ R.T + t)).max() <= 1e-14


@pytest.mark.parametrize("name,pose", kc.CASES)
def test_restated_transform_has_the_right_direction(name, pose):
    """O_l (the mesh as given, asked at the restated q_l) against O_w (the mesh moved to the world,
    asked at Q_w): both within the exclusion cap, equal inside flags and closest points to
    1e-12 max(1, max|Q_w|) on the jointly kept queries."""
    V, F, R, t, Q_w, q_l, ol, ow = kc.case(name, pose)
    assert len(Q_w) == 2600
    both = ol.keep & ow.keep
    print(f"{name} {pose}: excluded {(~ol.keep).sum()} / jointly {(~both).sum()}, "
          f"max |R c_l + t - c_w| {np.abs(kc.to_world(R, t, ol.c) - ow.c)[both].max():.3e}")
    assert (~ol.keep).sum() <= mc.MAX_EXCLUDED * len(Q_w)
    assert (~both).sum() <= mc.MAX_EXCLUDED * len(Q_w)
    assert np.array_equal(ol.inside[both], ow.inside[both])
    assert ol.inside[both].any() and (~ol.inside[both]).any()
    assert np.abs(kc.to_world(R, t, ol.c) - ow.c)[both].max() <= 1e-12 * max(1.0, np.abs(Q_w).max())


def test_host_pose_validation(tmp_path):
    """tests/cpp/kinematic_pose.cpp: validate_mesh_pose accepts the three poses and refuses a
    reflection, a scaled rotation (1.001 R), a NaN and an infinity, each with ERR_ARG and a message
    naming the cause; apply_mesh_pose writes the row."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    path = tmp_path / "poses.txt"
    with open(path, "w") as f:
        for R, t in kc.POSES.values():
            f.write(" ".join(repr(float(v)) for v in list(R.reshape(9)) + list(t)) + "\n")
    exe = str(tmp_path / "kinematic_pose")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "kinematic_pose.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok 3 poses" in r.stdout, r.stdout + r.stderr


def test_spinning_torus_scene():
    sc = scenes.cloth_on_spinning_torus(n_steps=7, dtheta=0.05)
    base = scenes.cloth_on_torus(n_steps=7)
    assert sc.name == "cloth_on_spinning_torus" and np.array_equal(sc.x, base.x)
    assert base.mesh_obstacle_poses is None
    P = sc.mesh_obstacle_poses
    assert P.shape == (7, 1, 12) and not P[:, 0, 9:].any()
    for k in range(7):
        R = P[k, 0, :9].reshape(3, 3)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
        assert np.allclose(R, kc.rotation((0.0, 1.0, 0.0), 0.05 * (k + 1)), atol=1e-15)
        assert np.array_equal(R[1], [0.0, 1.0, 0.0])   # about the y axis
