"""Writes tests/golden/eigsym_jacobi/<name>.Lam.npy: the eigenvalues (descending, float64) of the four graded positive definite
inputs of tests/eigsym_jacobi_common.py, rounded from mpmath.eigsy at 60 digits. The float64 input is converted exactly, so the
reference is that of the matrix the tests use, not of the real-number construction. Needs mpmath (the tests do not).

    python tools/gen_golden_eigsym_jacobi.py
"""
import os
import sys

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import eigsym_jacobi_common as jc  # noqa: E402


def main():
    mpmath.mp.dps = 60
    os.makedirs(jc.GOLDEN, exist_ok=True)
    for name, (seed, N, span) in jc.GRADED.items():
        S = jc.graded_pd(seed, N, span)
        assert np.array_equal(S, S.T)
        M = mpmath.matrix(N, N)
        for i in range(N):
            for j in range(N):
                M[i, j] = mpmath.mpf(float(S[i, j]))
        ev = mpmath.eigsy(M, eigvals_only=True)
        lam = np.array(sorted((float(x) for x in ev), reverse=True), dtype=np.float64)
        np.save(os.path.join(jc.GOLDEN, name + ".Lam.npy"), lam)
        print("%s: N = %d, cond ~ %.1e, lambda in [%.3e, %.3e]" % (name, N, lam[0] / lam[-1], lam[-1], lam[0]), flush=True)


if __name__ == "__main__":
    main()
