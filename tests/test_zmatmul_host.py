"""CPU checks of complex matmul2 / matmul: the reference's argument errors are raised for complex operands before any device
work, unsupported dtypes are refused, the C ABI rejects bad arguments of nd4hip_zgemm_batched, nothing is computed without a
GPU, and the golden fixtures of tests/golden/zmatmul are consistent with the generator they name."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from nd4js_amd import _lib, la, rng

ZDIR = os.path.join(GOLDEN, "zmatmul")
Z = np.ones((3, 3), dtype=np.complex128)


@pytest.fixture
def no_device(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "handle", fail)


def test_abi_exports_the_zgemm_entry_points():
    lib = _lib.load()
    for f in ("nd4hip_zgemm_batched", "nd4hip_zgemm_batched_dev"):
        assert hasattr(lib, f) and f in _lib.SIGNATURES


@pytest.mark.parametrize("other", [np.ones((3, 3)), np.ones((3, 3), dtype=np.int32), Z])
def test_reference_errors_for_complex_operands(no_device, other):
    for a, b in ((Z, other), (other, Z)):
        with pytest.raises(ValueError, match=r"^A must be at least 2D\.$"):
            la.matmul2(a[0], b)
        with pytest.raises(ValueError, match=r"^B must be at least 2D\.$"):
            la.matmul2(a, b[0])
        with pytest.raises(ValueError, match=r"^The last dimension of A and the 2nd to last dimension of B do not match\.$"):
            la.matmul2(a[:, :2], b)
        with pytest.raises(ValueError, match=r"^Shapes are not broadcast-compatible\.$"):
            la.matmul2(np.broadcast_to(a, (2, 3, 3)), np.broadcast_to(b, (3, 3, 3)))
    with pytest.raises(ValueError, match=r"^Shape mismatch\.$"):
        la.matmul(Z, Z, np.ones((2, 2), dtype=np.complex128))


def test_out_must_be_complex128(no_device):
    with pytest.raises(ValueError, match="C-contiguous complex128"):
        la.matmul2(Z, Z, out=np.empty((3, 3)))
    with pytest.raises(ValueError, match="C-contiguous complex128"):
        la.matmul2(Z, np.ones((3, 3)), out=np.empty((3, 3), dtype=np.complex128)[:, :2])


def test_unsupported_complex_pairings_are_refused(no_device):
    with pytest.raises(TypeError, match="complex128"):
        la.matmul2(np.ones((2, 2), dtype=np.complex64), np.ones((2, 2), dtype=np.complex64))
    with pytest.raises(TypeError, match="complex128"):
        la.matmul2(Z, np.ones((3, 3), dtype=np.complex64))
    with pytest.raises(TypeError):
        la.matmul2(np.ones((3, 3), dtype=np.float32), Z)
    with pytest.raises(TypeError):
        la.matmul2(Z, np.ones((3, 3), dtype=np.float32))
    with pytest.raises(TypeError):
        la.matmul(Z, np.ones((3, 3), dtype=np.float32), Z)


def _zgemm(ac, bc, batch, I, K, J, sA, sB):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = _lib.load().nd4hip_zgemm_batched(None, ac, bc, batch, I, K, J, p, sA, p, sB, p)
    return rc, _lib.load().nd4hip_last_error().decode()


def test_abi_rejects_bad_arguments_before_the_handle():
    assert _zgemm(0, 0, 1, 2, 2, 2, 0, 0) == (-1, "nd4hip_zgemm_batched: at least one operand must be complex")
    for args in ((-1, 2, 2, 2), (1, -2, 2, 2), (1, 2, -2, 2), (1, 2, 2, -2)):
        assert _zgemm(1, 1, *args, 0, 0) == (-1, "nd4hip_zgemm_batched: negative extent")
    assert _zgemm(1, 0, 2, 2, 3, 4, 5, 0) == (-1, "nd4hip_zgemm_batched: strideA must be 0 or >= I*K")
    assert _zgemm(0, 1, 2, 2, 3, 4, 0, 11) == (-1, "nd4hip_zgemm_batched: strideB must be 0 or >= K*J")
    assert _zgemm(1, 1, 1, 2, 2, 2, 0, 0) == (-1, "nd4hip_zgemm_batched: NULL handle")      # valid arguments: the handle is next


@pytest.mark.skipif(_lib.load().nd4hip_device_count() > 0, reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    for a, b in ((Z, Z), (Z, np.eye(3)), (np.eye(3), Z), (np.eye(3, dtype=np.int32), Z)):
        with pytest.raises(_lib.Nd4HipError) as e:
            la.matmul2(a, b)
        assert e.value.code == -4 and "no HIP device" in str(e.value)
    with pytest.raises(_lib.Nd4HipError):
        la.matmul(Z, Z, Z)


# ---- the fixtures: inputs regenerate bit for bit from their seeds, and the reference's results agree with numpy's products
def _manifest():
    with open(os.path.join(ZDIR, "manifest.json")) as f:
        return json.load(f)


def regenerate(op):
    n = int(np.prod(op["shape"]))
    if op["dtype"] == "complex128":
        return rng.fill_uniform(op["seed"], 2 * n).view(np.complex128).reshape(op["shape"])
    u = rng.fill_uniform(op["seed"], n).reshape(op["shape"])
    return u if op["dtype"] == "float64" else np.trunc(u * 1000).astype(np.int32)


def test_fixture_inputs_match_the_generator():
    m = _manifest()
    assert m["rng"] == "fmix32-v1"
    seen = 0
    for meta in m["cases"].values():
        for key in ("A", "B"):
            op = meta[key]
            if "seed" in op and "file" in op:
                stored = np.load(os.path.join(ZDIR, op["file"]))
                assert stored.dtype == np.dtype(op["dtype"]) and np.array_equal(stored, regenerate(op))
                seen += 1
    assert seen >= 40


def test_fixture_results_agree_with_numpy_where_finite():
    cases = _manifest()["cases"]
    pairings = set()
    for name, meta in cases.items():
        A = np.load(os.path.join(ZDIR, meta["A"]["file"])) if "file" in meta["A"] else None
        B = np.load(os.path.join(ZDIR, meta["B"]["file"])) if "file" in meta["B"] else None
        if A is None or B is None or not (np.isfinite(A).all() and np.isfinite(B).all()):
            continue
        C = np.load(os.path.join(ZDIR, meta["C"]))
        ref = np.matmul(A.astype(np.complex128) if A.dtype == np.int32 else A, B.astype(np.float64) if B.dtype == np.int32 else B)
        assert C.dtype == np.complex128 and C.shape == ref.shape, name
        assert np.linalg.norm((C - ref).ravel()) <= 1e-13 * max(np.linalg.norm(ref.ravel()), 1e-300), name
        pairings.add(meta["pairing"])
    assert pairings == {"CC", "CR", "RC", "CI", "IC"}
