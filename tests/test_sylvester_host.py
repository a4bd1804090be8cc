"""schur_sylvester, sylvester_solve and lyapunov_solve: what la and dev refuse before the library is entered (no GPU needed), and the
names of the C entry points."""
import numpy as np
import pytest

from nd4js_amd import _lib, la

NAMES = ("schur_sylvester", "sylvester_solve", "lyapunov_solve")


def args(name, M, N, dtype=np.float64, lead=(), zeros=np.zeros):
    a, b, c = zeros(lead + (M, M), dtype=dtype), zeros(lead + (N, N), dtype=dtype), zeros(lead + (M, N), dtype=dtype)
    return (a, c) if name == "lyapunov_solve" else (a, b, c)


@pytest.mark.parametrize("name", NAMES)
def test_la_refuses_before_the_library(name):
    fn = getattr(la, name)
    with pytest.raises(TypeError, match=r"%s\(.*\): \w+\.dtype must be float64; complex" % name):
        fn(*args(name, 3, 3, np.complex128))
    with pytest.raises(TypeError, match="only float64 runs on the GPU path, got float32"):
        fn(*args(name, 3, 3, np.float32))
    with pytest.raises(ValueError, match="quadratic"):
        fn(np.zeros((4, 3)), *args(name, 3, 3)[1:])
    with pytest.raises(ValueError, match=r"must be \[\.\.\., 3, 3\]"):
        fn(*args(name, 3, 3)[:-1], np.zeros((3, 4)))
    with pytest.raises(ValueError, match="N <= 2048"):
        fn(*args(name, 2049, 2049))
    with pytest.raises(ValueError, match="broadcast-compatible"):
        fn(np.zeros((2, 3, 3)), *args(name, 3, 3, lead=(3,))[1:])
    assert fn(*args(name, 3, 3, lead=(0,))).shape == (0, 3, 3)   # no members: no handle is taken


def test_la_refuses_two_subdiagonal_entries_in_a_row():
    T = np.eye(4) + np.diag([1.0, 1.0, 0.0], -1)
    for ops in ((T, np.eye(2), np.zeros((4, 2))), (np.eye(2), T, np.zeros((2, 4)))):
        with pytest.raises(ValueError, match="not quasi-triangular"):
            la.schur_sylvester(*ops)


@pytest.mark.parametrize("name", NAMES)
def test_dev_refuses_alike(name):
    import torch
    from nd4js_amd import dev
    fn = getattr(dev, name)
    with pytest.raises(TypeError, match="must be float64; complex"):
        fn(*args(name, 2, 2, torch.complex128, zeros=torch.zeros))
    with pytest.raises(TypeError, match="got torch.float32"):
        fn(*args(name, 2, 2, torch.float32, zeros=torch.zeros))
    with pytest.raises(TypeError, match="float64 CUDA tensor"):
        fn(*args(name, 2, 2, torch.float64, zeros=torch.zeros))


def test_entry_points_are_named_by_form():
    lib = _lib.load()
    for op in ("nd4hip_dtrsyl_batched", "nd4hip_dgesyl_batched"):
        assert all(hasattr(lib, op + form) and op + form in _lib.SIGNATURES for form in ("_dev", "_host"))
        assert not hasattr(lib, op) and op not in _lib.SIGNATURES
