"""Writes tests/golden/hegv/: per catalogue case of tests/hegv_common.py, LAPACK's eigenvalues of A x = lambda B x for Hermitian A and
Hermitian positive definite B (scipy.linalg.eigh(A, B), descending) as <case>.Lam.npy. The inputs are regenerated from their seeds by
the tests; only the values are committed. Needs scipy; no test needs it.   python tools/gen_golden_hegv.py"""
import os
import sys

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import hegv_common as G  # noqa: E402


def lapack_values(A, B):
    lam = np.empty(A.shape[:-1])
    N = A.shape[-1]
    for out, (a, b) in zip(lam.reshape(-1, N), G.members(A, B)):
        out[:] = scipy.linalg.eigh(a, b, eigvals_only=True)[::-1]
    return lam


def main():
    os.makedirs(G.GOLDEN, exist_ok=True)
    for name in G.NAMES:
        A, B = G.inputs(name)
        np.save(os.path.join(G.GOLDEN, name + ".Lam.npy"), lapack_values(A, B))
    print("wrote %d cases to %s" % (len(G.NAMES), G.GOLDEN))


if __name__ == "__main__":
    main()
