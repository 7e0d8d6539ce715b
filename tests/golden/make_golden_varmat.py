"""Generates the per-element material fixtures under tests/golden/varmat/ from the REFERENCE itself.

Each scene of tests/varmat_cases.py (one group, 8 material levels assigned at random per element)
is expanded with scenes.per_element_groups into the reference's own layout -- one EnergyTerm per
element, each with its Lame -- and run through the reference drivers (make_golden.run_ref). Stored:
the inputs with the per-element E / nu / limit arrays and the reference's prim, comb, reject, x, v of
every step (data only). Run in the build container:

    make -C oracle ref && python tests/golden/make_golden_varmat.py
"""
from __future__ import annotations

import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the repository, tests/ and oracle/ on sys.path)
import varmat_cases  # noqa: E402

scenes = make_golden.scenes


def main(only=None):
    os.makedirs(varmat_cases.VARMAT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, sc in varmat_cases.cases().items():
            if only and name not in only:
                continue
            steps = make_golden.run_ref(scenes.per_element_groups(sc), tmp)
            varmat_cases.save(os.path.join(varmat_cases.VARMAT, name + ".npz"), sc, steps)
            print(name, [len(s["prim"]) for s in steps], "rejects", [int(sum(s["reject"])) for s in steps])


if __name__ == "__main__":
    main(sys.argv[1:])
