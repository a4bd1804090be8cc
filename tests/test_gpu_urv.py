"""URV (complete orthogonal decomposition) and its minimum-norm least squares on the GPU, through the C ABI: A = U R V,
R = [[T, 0], [0, 0]] with exact zeros outside T, U and V orthogonal, T and V[:r] against the reference's fixtures up to
signs, and urv_lstsq against the fixtures, numpy's pseudo-inverse and the device's own svd_lstsq."""
import numpy as np
import pytest

from nd4js_amd import la
from srrqr_common import input_of, load, manifest, y_of

pytestmark = pytest.mark.gpu

CASES = manifest()
URV = sorted(k for k, v in CASES.items() if v["op"] == "urv_decomp_full")
URVLS = sorted(k for k, v in CASES.items() if v["op"] == "urv_lstsq")


def _mats(x):
    return x.reshape((-1,) + x.shape[-2:])


@pytest.mark.parametrize("name", URV)
def test_urv_matches_reference(name):
    meta = CASES[name]
    A = input_of(meta)
    U, R, V, r = la.urv_decomp_full(A)
    np.testing.assert_array_equal(r, load(meta, "r"))
    M, N = A.shape[-2:]
    for a, u, rr, v, rk, rg, vg in zip(_mats(A), _mats(U), _mats(R), _mats(V), np.ravel(r), _mats(load(meta, "R")), _mats(load(meta, "V"))):
        nA = max(np.linalg.norm(a), 1)
        assert np.abs(u @ rr @ v - a).max() <= 1e-13 * nA
        assert np.abs(u.T @ u - np.eye(M)).max() <= 1e-13
        assert np.abs(v @ v.T - np.eye(N)).max() <= 1e-13
        T = rr[:rk, :rk]
        out = rr.copy()
        out[:rk, :rk] = 0
        assert np.all(out == 0) and np.all(np.tril(T, -1) == 0)            # exact zeros outside the triangle T
        if rk == 0:
            continue
        # T = D1 Tg D2 and V[:r] = D2 Vg[:r] for sign matrices: D2 from the rows of V, D1 from the diagonal of T
        d2 = np.sign(np.sum(v[:rk] * vg[:rk], axis=1))
        d1 = np.sign(np.diag(T)) * np.sign(np.diag(rg[:rk, :rk])) * d2
        assert np.abs(d2[:, None] * v[:rk] - vg[:rk]).max() <= 1e-12
        assert np.abs(d1[:, None] * T * d2[None, :] - rg[:rk, :rk]).max() <= 1e-12 * np.abs(rg).max()


def test_urv_full_rank_square_is_a_permutation():
    meta = CASES["urv_dense_48x48"]
    A = input_of(meta)
    _, R, V, r = la.urv_decomp_full(A)
    assert int(r) == 48
    np.testing.assert_array_equal(V, load(meta, "V"))                       # V[i, P[i]] = 1 exactly


@pytest.mark.parametrize("name", URVLS)
def test_urv_lstsq_matches_reference_and_pinv(name):
    meta = CASES[name]
    A, y = input_of(meta), y_of(meta)
    x = la.urv_lstsq(la.urv_decomp_full(A), y)
    xg = load(meta, "x")
    np.testing.assert_allclose(x, xg, rtol=0, atol=1e-10 * np.abs(xg).max())
    if meta["family"] in ("rankdef", "lowrank"):                            # well separated: sigma_r / sigma_{r+1} > 1e10
        xp = np.linalg.pinv(A, rcond=1e-10) @ y
        np.testing.assert_allclose(x, xp, rtol=0, atol=1e-9 * np.abs(xp).max())


def test_urv_lstsq_matches_svd_lstsq_on_device():
    meta = CASES["urvls_rankdef_48"]
    A, y = input_of(meta), y_of(meta)
    U, sv, V = la.svd_decomp(A)
    xs = la.svd_lstsq(U, sv, V, y)
    x = la.urv_lstsq(*la.urv_decomp_full(A), y)                              # the five-argument form
    np.testing.assert_allclose(x, xs, rtol=0, atol=1e-9 * np.abs(xs).max())


def test_urv_lstsq_broadcasts_ranks_and_operands():
    meta = CASES["urvls_rankdef_48"]
    A, y = input_of(meta), y_of(meta)
    U, R, V, r = la.urv_decomp_full(A)
    Y = np.stack([y, 2 * y, -y])
    X = la.urv_lstsq(U, R, V, r, Y)                                         # U, R, V, ranks broadcast over Y's batch
    x = la.urv_lstsq(U, R, V, r, y)
    np.testing.assert_allclose(X, np.stack([x, 2 * x, -x]), rtol=0, atol=1e-12 * np.abs(x).max())
    Xr = la.urv_lstsq(U, R, V, np.array([int(r), 1, 0], dtype=np.int32), y)  # ranks alone carries the batch
    assert Xr.shape == (3,) + x.shape
    np.testing.assert_array_equal(Xr[0], x)
    assert np.all(Xr[2] == 0) and np.linalg.norm(Xr[1]) > 0


def test_urv_batch_equals_members_and_dev_form():
    torch = pytest.importorskip("torch")
    from nd4js_amd import dev
    meta = CASES["urv_batch3x20"]
    A = input_of(meta)
    out = la.urv_decomp_full(A)
    for b in range(A.shape[0]):
        for x, y in zip(out, la.urv_decomp_full(A[b])):
            np.testing.assert_array_equal(x[b], y)
    U, R, V, r = dev.urv_decomp_full(torch.from_numpy(A).cuda())
    for x, y in zip((U, R, V, r), out):
        np.testing.assert_array_equal(x.cpu().numpy(), y)
    Y = torch.from_numpy(np.stack([y_of({"shape": [20, 20], "J": 2, "y_seed": 5})] * 3)).cuda()
    X = dev.urv_lstsq(U, R, V, r, Y)
    torch.cuda.synchronize()
    np.testing.assert_allclose(X.cpu().numpy(), la.urv_lstsq(out[0], out[1], out[2], out[3], Y.cpu().numpy()), rtol=0, atol=1e-12)
