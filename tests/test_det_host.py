"""CPU checks of det, slogdet, det_tri, slogdet_tri, rank, lstsq and norm: the reference's argument errors (det.js, norm.js) are
raised before any device work, and the C ABI exports the new entry points."""
import numpy as np
import pytest

from nd4js_amd import _lib, la

NAMES = ["nd4hip_ddet_batched", "nd4hip_dslogdet_batched", "nd4hip_ddettri_batched", "nd4hip_dslogdettri_batched", "nd4hip_dnrmfro"]


@pytest.fixture
def no_device(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "handle", fail)


def test_abi_exports_the_det_and_norm_entry_points():
    lib = _lib.load()
    for n in NAMES:
        for f in (n, n + "_dev"):
            assert hasattr(lib, f) and f in _lib.SIGNATURES


def test_det_errors_before_device_work(no_device):
    with pytest.raises(ValueError, match=r"^qr_decomp\(A\): A\.ndim must be at least 2\.$"):
        la.det(np.ones(3))
    with pytest.raises(ValueError, match=r"^qr_decomp\(A\): A\.ndim must be at least 2\.$"):
        la.slogdet(np.ones(3))
    with pytest.raises(ValueError, match=r"^det_tri\(a\): a must be square matrices\.$"):
        la.det(np.ones((3, 5)))
    with pytest.raises(ValueError, match=r"^det_tri\(A\): A must be square matrices\.$"):
        la.slogdet(np.ones((2, 3, 5)))


def test_det_tri_errors_before_device_work(no_device):
    with pytest.raises(ValueError, match=r"^det_tri\(a\): a\.shape=\[2\]; a\.ndim must be at least 2\.$"):
        la.det_tri(np.ones(2))
    with pytest.raises(ValueError, match=r"^det_tri\(A\): A\.ndim must be at least 2\.$"):
        la.slogdet_tri(np.ones(2))
    with pytest.raises(ValueError, match=r"^det_tri\(a\): a must be square matrices\.$"):
        la.det_tri(np.ones((5, 4)))
    with pytest.raises(ValueError, match=r"^det_tri\(A\): A must be square matrices\.$"):
        la.slogdet_tri(np.ones((4, 5)))


def test_norm_errors_before_device_work(no_device):
    with pytest.raises(ValueError, match=r"^norm\(A,ord,axis\): Unsupported ord: inf\.$"):
        la.norm(np.ones(3), "inf")
    with pytest.raises(ValueError, match=r"^norm\(A,ord,axis\): Unsupported ord: 2\.$"):
        la.norm(np.ones(3), 2)
    with pytest.raises(ValueError, match=r"^norm\(A,ord,axis\): axis argument not yet supported\.$"):
        la.norm(np.ones((3, 3)), "fro", 0)


def test_non_float64_is_refused_not_computed_on_the_cpu(no_device):
    with pytest.raises(TypeError):
        la.det(np.ones((3, 3), dtype=np.float32))


@pytest.mark.skipif(_lib.load().nd4hip_device_count() > 0, reason="GPU present")
def test_det_fails_loudly_without_gpu():
    for fn in (la.det, la.slogdet, la.det_tri, la.slogdet_tri, la.norm):
        with pytest.raises(_lib.Nd4HipError):
            fn(np.eye(3))
