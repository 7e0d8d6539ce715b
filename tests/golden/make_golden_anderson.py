"""Generates tests/golden/anderson.npz from the REFERENCE's own AndersonAcceleration class
(admm_anderson_hard_zxu/src/AndersonAcceleration.h), driven by op 5 of oracle/_ref/ref_element:
init(u0), then T = 2 m + 3 calls of compute(G_k, u), the u of every call stored. Data only.

The G sequences are those of the float64 port on the case's contraction (G_k = A u_k + b with the
port's own u_k): the class, fed the same G_k, follows the port to rounding, so the sequence is the
fixed-point iteration's own.

    make -C oracle ref && python tests/golden/make_golden_anderson.py
"""
from __future__ import annotations

import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import anderson_cases as ac  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref")
# The class is fed a recorded G sequence, not the map: a rounding difference in u_k is not fed back
# through G. It then grows or decays by about |dG| / |dF| <= rho / (1 - rho) a step, so rho = 0.5
# (not the GPU cases' 0.9) keeps the recorded chains comparable over all 2 m + 3 steps.
RHO = 0.5
CHAINS = {"m3": (3, 40, 40, 11), "m6": (6, 64, 41, 12), "m20": (20, 63, 63, 13)}   # m, dim, eff, seed


def main():
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (m, dim, eff, seed) in CHAINS.items():
            f = ac.Contraction(dim, seed, RHO)
            st = ac.clean_state(m, eff, dim - eff, eff, f.u0)
            T = 2 * m + 3
            G = np.zeros((T, dim))
            for k in range(T):
                G[k] = f(st["cur"])
                _, st = ac.port_step(st, G[k])
            buf = struct.pack("<ii", 5, 1) + struct.pack("<4d", m, dim, eff, T) + f.u0.astype("<f8").tobytes() + G.astype("<f8").tobytes()
            pin, pout = os.path.join(tmp, "aa.bin"), os.path.join(tmp, "aa.out")
            with open(pin, "wb") as fh:
                fh.write(buf)
            r = subprocess.run([os.path.join(REF, "ref_element"), pin, pout], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(r.stderr)
            u = np.fromfile(pout, dtype="<f8").reshape(T, dim)
            arrays.update({f"{name}_m": np.int32(m), f"{name}_eff": np.int32(eff), f"{name}_u0": f.u0, f"{name}_G": G, f"{name}_u": u})
    out = os.path.join(HERE, "anderson.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
