"""inv, tril_inv, triu_inv and cholesky_inv: what la and dev refuse before the library is entered (no GPU needed)."""
import numpy as np
import pytest

from nd4js_amd import la

NAMES = ("inv", "tril_inv", "triu_inv", "cholesky_inv")


@pytest.mark.parametrize("name", NAMES)
def test_la_refuses_before_the_library(name):
    fn = getattr(la, name)
    with pytest.raises(TypeError, match=r"%s\(\w\): \w\.dtype must be float64; complex" % name):
        fn(np.eye(3, dtype=np.complex128))
    with pytest.raises(TypeError, match="only float64 runs on the GPU path, got float32"):
        fn(np.eye(3, dtype=np.float32))
    for bad, text in ((np.ones((4, 3)), "quadratic"), (np.ones(4), "at least 2"), (np.zeros((2049, 2049)), "N <= 2048")):
        with pytest.raises(ValueError, match=text):
            fn(bad)
    assert fn(np.zeros((0, 3, 3))).shape == (0, 3, 3)           # no members: no handle is taken


@pytest.mark.parametrize("name", NAMES)
def test_dev_refuses_alike(name):
    import torch
    from nd4js_amd import dev
    fn = getattr(dev, name)
    with pytest.raises(TypeError, match="must be float64; complex"):
        fn(torch.zeros((2, 2), dtype=torch.complex128))
    with pytest.raises(TypeError, match="got torch.float32"):
        fn(torch.zeros((2, 2), dtype=torch.float32))
    with pytest.raises(TypeError, match="contiguous float64 CUDA tensor"):
        fn(torch.zeros((2, 2), dtype=torch.float64))
