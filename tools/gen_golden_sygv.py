"""Writes tests/golden/sygv/: manifest.json and, per catalogue case of tests/sygv_common.py, LAPACK's eigenvalues of A x = lambda B x
(scipy.linalg.eigh(A, B), descending) as <case>.Lam.npy. The inputs are regenerated from their seeds by the tests; only the values
and the Frobenius norms of the inputs are committed. Needs scipy; no test needs it.   python tools/gen_golden_sygv.py"""
import json
import os
import sys

import numpy as np
import scipy
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sygv_common as G  # noqa: E402


def lapack_values(A, B):
    lam = np.empty(A.shape[:-1])
    N = A.shape[-1]
    for out, (a, b) in zip(lam.reshape(-1, N), G.members(A, B)):
        out[:] = scipy.linalg.eigh(a, b, eigvals_only=True)[::-1]
    return lam


def main():
    os.makedirs(G.GOLDEN, exist_ok=True)
    cases = {}
    for name in G.NAMES:
        A, B = G.inputs(name)
        np.save(os.path.join(G.GOLDEN, name + ".Lam.npy"), lapack_values(A, B))
        cases[name] = {"shape_A": list(A.shape), "shape_B": list(B.shape),
                       "fro_A": [float(np.linalg.norm(a)) for a, _ in G.members(A, B)],
                       "fro_B": [float(np.linalg.norm(b)) for _, b in G.members(A, B)]}
    with open(os.path.join(G.GOLDEN, "manifest.json"), "w") as f:
        json.dump({"generator": "tools/gen_golden_sygv.py", "reference": "scipy.linalg.eigh(A, B), scipy %s" % scipy.__version__,
                   "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(cases), G.GOLDEN))


if __name__ == "__main__":
    main()
