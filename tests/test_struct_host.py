"""The structure functions without a device: the fixtures of tests/golden/struct against their manifest, the numpy restatement
of tests/struct_common.py against EVERY fixture bit for bit (which is what entitles tests/test_gpu_struct.py to use it on shapes
that have no fixture), and every call the reference refuses, through la.*, with the recorded text and before any device work."""
import os

import numpy as np
import pytest

import struct_common as sc
from nd4js_amd import _lib, la

ABI = ["nd4hip_dtranspose_batched", "nd4hip_dtri_batched", "nd4hip_ddiag_batched", "nd4hip_ddiagmat_batched", "nd4hip_dpermute_batched"]


# ------------------------------------------------------------------------------------------------ the fixtures themselves
def test_manifest_matches_the_files():
    entries = list(sc.INPUTS.values()) + [c["out"] for c in sc.CASES.values()]
    assert len({e["file"] for e in entries}) == len(entries)
    for e in entries:
        assert os.path.getsize(os.path.join(sc.DIR, e["file"])) <= sc.SIZE_LIMIT, e["file"]
        assert sc.sha256(e) == e["sha256"], e["file"]
        a = sc.load(e)
        assert list(a.shape) == e["shape"] and a.dtype == np.dtype(e["dtype"]), e["file"]
    on_disk = {f for f in os.listdir(sc.DIR) if f.endswith(".npy")}
    assert on_disk == {e["file"] for e in entries}


def test_fixtures_cover_every_function_and_the_hard_values():
    assert {c["fn"] for c in sc.CASES.values()} == set(sc.NAMES)
    assert {e["fn"] for e in sc.ERRORS} == set(sc.NAMES) - {"transpose"}
    for name in ("A_5x8", "A_8x5", "A_130x67", "A_65x130"):
        a = sc.load(sc.INPUTS[name])
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
        assert ((a == 0) & np.signbit(a)).any() and ((a != 0) & (np.abs(a) < 2.0 ** -1022)).any()
    a = sc.load(sc.INPUTS["A_5x8"])                     # NaN and -0 on both sides of the cut
    assert np.isnan(a[1, 0]) and np.isnan(a[1, 2]) and np.signbit(a[0, 1]) and np.signbit(a[2, 1])
    for fn in ("unpermute_rows", "unpermute_cols"):       # zero rows / columns and overwritten ones are really there
        dup = [c for c in sc.CASES.values() if c["fn"] == fn and c["kind"] == "dup"]
        assert dup and all(c["unnamed"] > 0 and c["twice"] > 0 for c in dup if sc.INPUTS[c["args"]["P"]]["shape"][-1] >= 33)
    # both sides of the length an inverse map may have in LDS (csrc/struct.hip: STRUCT_LDS_MAP = 4096)
    lengths = {sc.INPUTS[c["args"]["P"]]["shape"][-1] for c in sc.CASES.values() if "P" in c["args"]}
    assert min(lengths) == 1 and 130 in lengths and max(lengths) > 4096


# ------------------------------------------------------------------------------------------------ restatement against fixtures
@pytest.mark.parametrize("name", sc.ALL)
def test_restatement_reproduces_the_fixture(name):
    fn, args, want = sc.case(name)
    got = sc.RESTATED[fn](*args)
    assert got.shape == want.shape, name
    assert np.array_equal(np.isnan(got), np.isnan(want)) and sc.same_bits(got, want), name


def test_restatement_last_writer_and_zero_rows():
    A = np.arange(1.0, 13.0).reshape(4, 3)
    P = np.array([2, 0, 2, 0], dtype=np.int32)
    B = sc.unpermute_rows(A, P)
    assert np.array_equal(B, np.array([A[3], [0, 0, 0], A[2], [0, 0, 0]]))
    assert not np.signbit(B[1]).any()
    Bc = sc.unpermute_cols(A.T.copy(), P)
    assert np.array_equal(Bc, B.T)
    assert sc.permute_rows(A, np.zeros((2, 1, 4), dtype=np.int32)).shape == (2, 1, 4, 3)


# ------------------------------------------------------------------------------------------------ refused calls
@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a refused call reached the device")
    monkeypatch.setattr(_lib, "handle", refuse)


@pytest.mark.parametrize("i", [i for i, e in enumerate(sc.ERRORS) if not e.get("on_device")])
def test_refused_before_any_device_work(i, no_device):
    e = sc.ERRORS[i]
    kind = TypeError if "dtype" in e["message"] else ValueError
    with pytest.raises(kind) as info:
        getattr(la, e["fn"])(*sc.refused_call(e))
    assert str(info.value) == e["message"]


def test_dtypes_are_refused_not_converted(no_device):
    for fn in ("transpose", "tril", "triu", "diag", "diag_mat"):
        with pytest.raises(TypeError, match="only float64"):
            getattr(la, fn)(np.zeros((3, 3), dtype=np.float32))
    for fn in sc.PERM:
        with pytest.raises(TypeError, match="only float64"):
            getattr(la, fn)(np.zeros((3, 3), dtype=np.int32), np.arange(3, dtype=np.int32))
        with pytest.raises(TypeError) as info:
            getattr(la, fn)(np.zeros((3, 3)), np.arange(3, dtype=np.int64))
        assert str(info.value) == '%s(A,P): P.dtype must be "int32".' % fn
    assert la.transpose(np.arange(3.0)).shape == (3,)            # fewer than two axes: the array itself, like NDArray.T


def test_abi_lists_the_entry_points():
    for name in ABI:
        assert name in _lib.SIGNATURES and name + "_dev" in _lib.SIGNATURES
