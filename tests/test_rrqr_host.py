"""Column-pivoted QR (rrqr_decomp & co., src/la/rrqr.js) without a GPU: the fixtures are consistent with their regenerated
inputs, and the host wrappers exist and check their arguments with the reference's messages before any device work."""
import numpy as np
import pytest

from nd4js_amd import _lib, la
from rrqr_common import load, make, manifest

CASES = manifest()
DECOMP = sorted(k for k, v in CASES.items() if v["op"] == "rrqr_decomp" and not v.get("sampled"))


@pytest.mark.parametrize("name", DECOMP)
def test_fixture_reproduces_its_input(name):
    meta = CASES[name]
    A = make(meta["seed"], meta["shape"], meta["family"])
    Q, R, P = load(meta, "Q"), load(meta, "R"), load(meta, "P")
    assert P.dtype == np.int32 and P.shape == A.shape[:-2] + A.shape[-1:]
    Ap = np.take_along_axis(A, P[..., None, :].astype(np.int64).repeat(A.shape[-2], axis=-2), axis=-1)
    err = np.linalg.norm(Ap - Q @ R) / max(np.linalg.norm(A), 1e-300)
    assert err <= 1e-14, err
    assert np.all(np.sort(P, axis=-1) == np.arange(A.shape[-1]))


def test_fixture_large_cases_are_permutations():
    for name in ("large1024", "large2048"):
        meta = CASES[name]
        P = load(meta, "P")
        assert np.array_equal(np.sort(P), np.arange(P.size))
        d = np.abs(load(meta, "Rdiag"))
        assert np.all(d[1:] <= d[:-1] * (1 + 1e-12))


def test_wrappers_exist():
    for n in ("rrqr_decomp", "rrqr_decomp_full", "rrqr_rank", "rrqr_lstsq", "rrqr_solve", "solve", "SingularMatrixSolveError"):
        assert hasattr(la, n), n
    e = la.SingularMatrixSolveError(np.zeros((2, 1)))
    assert isinstance(e, ValueError) and e.x.shape == (2, 1)
    for n in ("nd4hip_dgeqp3_batched", "nd4hip_dgeqp3_full_batched", "nd4hip_dqp3rank_batched", "nd4hip_dqp3ls_batched"):
        assert n in _lib.SIGNATURES and n + "_dev" in _lib.SIGNATURES


def test_argument_checks_use_the_reference_text():
    def msg(fn, *a):
        with pytest.raises(ValueError) as e:
            fn(*a)
        return str(e.value)
    Q, R, P, y = np.eye(3), np.eye(3), np.arange(3, dtype=np.int32), np.ones((3, 1))
    assert msg(la.rrqr_decomp, np.ones(3)) == "A must be at least 2D."
    assert msg(la.rrqr_decomp_full, np.ones(3)) == "A must be at least 2D."
    assert msg(la.rrqr_lstsq, (Q, R, P), y, P) == "rrqr_lstsq(Q,R,P, y): Either 2 ([Q,R,P], y) or 4 arguments (Q,R,P, y) expected."
    assert msg(la.rrqr_lstsq, np.ones(3), R, P, y) == "rrqr_lstsq(Q,R,P, y): Q.ndim must be at least 2."
    assert msg(la.rrqr_lstsq, Q, np.ones(3), P, y) == "rrqr_lstsq(Q,R,P, y): R.ndim must be at least 2."
    assert msg(la.rrqr_lstsq, Q, R, np.int32(0), y) == "rrqr_lstsq(Q,R,P, y): P.ndim must be at least 1."
    assert msg(la.rrqr_lstsq, Q, R, P, np.ones(3)) == "rrqr_lstsq(Q,R,P, y): y.ndim must be at least 2."
    assert msg(la.rrqr_lstsq, Q, R, P.astype(np.float64), y) == 'rrqr_lstsq(Q,R,P, y): P.dtype must be "int32".'
    assert msg(la.rrqr_lstsq, Q, R, P, np.ones((4, 1))) == "rrqr_lstsq(Q,R,P,y): Q and y don't match."
    assert msg(la.rrqr_lstsq, Q, np.eye(4)[:, :3], P, y) == "rrqr_lstsq(Q,R,P,y): Q and R don't match."
    assert msg(la.rrqr_lstsq, Q, R, np.arange(2, dtype=np.int32), y) == "rrqr_lstsq(Q,R,P,y): R and P don't match."
    assert msg(la.rrqr_lstsq, np.ones((2, 3, 3)), R, P, np.ones((3, 3, 1))) == "rrqr_lstsq(Q,R,P,y): Q,R,P,y not broadcast-compatible."
    assert msg(la.rrqr_solve, np.ones((4, 3)), np.ones((3, 3)), P, np.ones((4, 1))) == "rrqr_solve(Q,R,P, y): Q @ R not square."
    assert msg(la.rrqr_rank, np.ones(3)) == "rrqr_rank(R): R.ndim must be at least 2."


@pytest.mark.skipif(_lib.load().nd4hip_device_count() > 0, reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    for fn, args in ((la.rrqr_decomp, (np.eye(4),)), (la.rrqr_decomp_full, (np.eye(4),)), (la.rrqr_rank, (np.eye(4),)),
                     (la.rrqr_lstsq, (np.eye(3), np.eye(3), np.arange(3, dtype=np.int32), np.ones((3, 1)))),
                     (la.solve, (np.eye(3), np.ones((3, 1))))):
        with pytest.raises(_lib.Nd4HipError) as e:
            fn(*args)
        assert e.value.code == -4 and "no HIP device" in str(e.value)
