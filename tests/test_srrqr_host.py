"""Strong RRQR without a GPU: the fixtures of tests/golden/srrqr/ against their regenerated inputs, the argument checks and
messages, and the new entry points in the header, the bindings and the N-API shim."""
import os

import numpy as np
import pytest

from nd4js_amd import la
from srrqr_common import EPS, input_of, load, manifest, strong_F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = manifest()


def test_manifest_files_exist():
    assert len(CASES) >= 30
    for name, meta in CASES.items():
        for f in meta["files"].values():
            assert os.path.exists(os.path.join(ROOT, "tests", "golden", "srrqr", f)), f


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if "Q" in v["files"]))
def test_golden_factorises_regenerated_input(name):
    meta = CASES[name]
    A = input_of(meta)
    Q, R, P, r = (load(meta, k) for k in ("Q", "R", "P", "r"))
    A2, Q2, R2 = (x.reshape((-1,) + x.shape[-2:]) for x in (A, Q, R))
    P2, r2 = P.reshape(-1, P.shape[-1]), r.reshape(-1)
    dtol = (meta["opt"] or {}).get("dtol", 1.01)
    for a, q, rr, p, rk in zip(A2, Q2, R2, P2, r2):
        assert sorted(p) == list(range(a.shape[1]))
        assert np.abs(q @ rr - a[:, p]).max() <= 1e-13 * max(np.linalg.norm(a), 1)
        assert np.all(np.triu(rr[:rk], 0)[:, :rk] == rr[:rk, :rk])           # R[:r] upper trapezoidal
        assert strong_F(rr, rk) <= dtol * (1 + 1e-8)


def test_kahan_fixture_shows_the_strong_rank():
    for name, n in (("kahan60", 60), ("kahan90", 90)):
        meta = CASES[name]
        assert int(load(meta, "r")) == n - 1
        assert meta["rrqr_rank"] == [n]
        sv = np.linalg.svd(input_of(meta), compute_uv=False)
        assert int(la.svd_rank(sv)) == n - 1


def test_user_ztol_is_in_units_of_the_norm():
    assert int(load(CASES["eye3_ztol2"], "r")) == 0


def test_argument_checks():
    with pytest.raises(ValueError, match=r"srrqr_decomp_full\(A,opt\): A must be at least 2D\."):
        la.srrqr_decomp_full(np.zeros(3))
    with pytest.raises(ValueError, match=r"Complex A not \(yet\) supported\."):
        la.srrqr_decomp_full(np.zeros((2, 2), dtype=complex))
    with pytest.raises(ValueError, match=r"srrqr_decomp_full\(A,opt\): Invalid opt\.dtol: 0\.5\. Must be >=1\."):
        la.srrqr_decomp_full(np.eye(2), {"dtol": 0.5})
    with pytest.raises(ValueError, match=r"Invalid opt\.dtol: NaN\. Must be >=1\."):
        la.srrqr_decomp_full(np.eye(2), dtol=float("nan"))
    with pytest.raises(ValueError, match=r"srrqr_decomp_full\(A,opt\): invalid opt\.ztol: -1\. Must be non-negative number\."):
        la.srrqr_decomp_full(np.eye(2), {"ztol": -1})
    with pytest.raises(ValueError, match=r"NDArray as opt\.dtol not yet supported\."):
        la.srrqr_decomp_full(np.eye(2), {"dtol": np.ones(1)})
    with pytest.raises(ValueError, match=r"NDArray as opt\.ztol not yet supported\."):
        la.srrqr_decomp_full(np.eye(2), {"ztol": np.ones(1)})


def test_rrqr_args_take_the_srrqr_four_tuple():
    Q, R, P, y = la._rrqr_args(("q", "r", "p", "rank"), "y", None, None)
    assert (Q, R, P, y) == ("q", "r", "p", "y")


def test_entry_points_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "nd4hip.h")) as f:
        hdr = f.read()
    from nd4js_amd import _lib
    with open(os.path.join(ROOT, "nd4js_amd", "csrc", "napi_shim.c")) as f:
        shim = f.read()
    for name in ("nd4hip_dsrrqr_batched", "nd4hip_dsrrqr_batched_dev"):
        assert name + "(" in hdr.replace(" ", "")
        assert name in _lib.SIGNATURES
    assert '"nd4hip_dsrrqr_batched"' in shim and '"dsrrqr_batched"' in shim


def test_reference_messages_before_the_device():
    with pytest.raises(ValueError, match=r"^Assertion failed\. Invalid dtol: Infinity\.$"):
        la.srrqr_decomp_full(np.eye(2), {"dtol": float("inf")})
    with pytest.raises(ValueError, match=r"^Assertion failed\. Invalid ztol: Infinity\.$"):
        la.srrqr_decomp_full(np.eye(2), {"ztol": float("inf")})
    with pytest.raises(ValueError, match=r"Either 2 \(\[U,R,V,ranks\], Y\) or 5 arguments"):
        la.urv_lstsq(np.eye(2), np.eye(2), np.eye(2))
    with pytest.raises(ValueError, match=r"urv_lstsq\(U,R,V, Y\): V\.ndim must be at least 2\."):
        la.urv_lstsq(np.eye(2), np.eye(2), np.ones(2), 2, np.eye(2))
    with pytest.raises(ValueError, match=r"Matrix dimensions incompatible\."):
        la.urv_lstsq(np.eye(2), np.eye(3), np.eye(3), 2, np.eye(2))
    with pytest.raises(ValueError, match=r"not broadcast-compatible\."):
        la.urv_lstsq(np.eye(2), np.eye(2), np.eye(2), np.zeros(3, np.int32), np.zeros((2, 2, 1)))


def test_urv_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "nd4hip.h")) as f:
        hdr = f.read().replace(" ", "")
    from nd4js_amd import _lib
    for name in ("nd4hip_durv_batched", "nd4hip_durv_batched_dev", "nd4hip_durvls_batched", "nd4hip_durvls_batched_dev"):
        assert name + "(" in hdr and name in _lib.SIGNATURES


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v["op"] == "urv_decomp_full"))
def test_urv_fixture_shape(name):
    meta = CASES[name]
    R, V, r = load(meta, "R"), load(meta, "V"), load(meta, "r")
    for rr, v, rk in zip(R.reshape((-1,) + R.shape[-2:]), V.reshape((-1,) + V.shape[-2:]), r.reshape(-1)):
        out = rr.copy(); out[:rk, :rk] = 0
        assert np.all(out == 0) and np.abs(v @ v.T - np.eye(v.shape[0])).max() < 1e-13
