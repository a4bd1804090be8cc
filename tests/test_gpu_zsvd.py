"""zbidiag_factor / zbidiag_apply_p / zsvd_decomp / zsvd_vals on the GPU (csrc/zgebrd.hip): la and dev give the same bits and leave their
operands untouched; the norm-wise bounds of DESIGN.md 4.28 with TOL = 1e-12, products formed in np.clongdouble, on the smallest
shapes at which each path can go wrong (tier A ends at 95 x 95). Largest shares measured: see DESIGN.md 4.28."""
import numpy as np
import pytest

import zlu_common as Z
from nd4js_amd import _lib, la
from test_gpu_zlu import _up, both

pytestmark = pytest.mark.gpu
TOL, L = 1e-12, np.clongdouble
NOCONV = r"%s\(A\): A contains NaN or Infinity\."


def gauss(shape, seed=1):
    r = np.random.default_rng(seed)
    return r.standard_normal(shape) + 1j * r.standard_normal(shape)


def fro(x):
    return float(np.sqrt(np.sum(np.abs(np.asarray(x, dtype=L)) ** 2)))


def H(x):
    return np.conj(np.swapaxes(x, -1, -2))


def bidiagonal(d, e):
    B = np.zeros(d.shape + d.shape[-1:], dtype=L)
    i = np.arange(d.shape[-1])
    B[..., i, i] = d
    B[..., i[:-1], i[1:]] = e
    return B


def check_bidiag(A):
    """bounds 1, 2 and 4 of a factorisation; returns it"""
    M, N = A.shape[-2:]
    F, tauq, taup, d, e = both("zbidiag_factor", A)
    assert d.dtype == e.dtype == np.float64 and d.shape == A.shape[:-2] + (N,) and e.shape == A.shape[:-2] + (N - 1,)
    assert np.isfinite(tauq).all() and np.isfinite(taup).all() and not taup[..., -1].any()
    Q = both("zqr_apply_q", F, tauq, np.broadcast_to(np.eye(M, N, dtype=np.complex128), A.shape).copy()).astype(L)
    P = both("zbidiag_apply_p", F, taup, np.broadcast_to(np.eye(N, dtype=np.complex128), A.shape[:-2] + (N, N)).copy()).astype(L)
    Zc = gauss(A.shape[:-2] + (N, 3), 5)
    Zc /= np.sqrt(np.sum(np.abs(Zc) ** 2, axis=-2, keepdims=True))
    back = both("zbidiag_apply_p", F, taup, both("zbidiag_apply_p", F, taup, Zc), True)
    for m in np.ndindex(A.shape[:-2]):
        s1 = fro(A[m] - Q[m] @ bidiagonal(d[m], e[m]) @ H(P[m])) / (TOL * max(fro(A[m]), 1e-300))
        s2 = max(fro(H(Q[m]) @ Q[m] - np.eye(N)), fro(H(P[m]) @ P[m] - np.eye(N))) / (TOL * np.sqrt(N))
        s2z = fro(back[m] - Zc[m]) / (TOL * np.sqrt(3))
        print("zbidiag_factor %s: shares of bounds 1, 2, 2 (P^H P Z): %.2e %.2e %.2e" % (A.shape, s1, s2, s2z))
        assert max(s1, s2, s2z) <= 1.0
    return F, tauq, taup, d, e


def sub(name, A, subset):
    """both() for a call with subset"""
    from nd4js_amd import dev
    keep, up = A.copy(), _up(A)
    out, outd = getattr(la, name)(A, subset=subset), getattr(dev, name)(up, subset=subset)
    assert Z.same_bits(A, keep) and Z.same_bits(up.cpu().numpy(), keep)
    for a, b in zip(out if isinstance(out, tuple) else (out,), outd if isinstance(outd, tuple) else (outd,)):
        assert Z.same_bits(a, b.cpu().numpy()), name + ": la and dev differ"
    return out


def check_triplets(A, U, sv, V, s_ref, i0=0):
    """bounds 1 - 3 on the triplets i0 .. i0 + k - 1 (bound 1 on A V^H = U diag(sv) when they are a subset)"""
    k = sv.shape[-1]
    for m in np.ndindex(A.shape[:-2]):
        Um, Vm, full = U[m].astype(L), V[m].astype(L), k == min(A.shape[-2:])
        r1 = A[m] - (Um * sv[m]) @ Vm if full else A[m] @ H(Vm) - Um * sv[m]
        s1 = fro(r1) / (TOL * max(fro(A[m]), 1e-300))
        s2 = max(fro(H(Um) @ Um - np.eye(k)), fro(Vm @ H(Vm) - np.eye(k))) / (TOL * np.sqrt(k))
        s3 = float(np.max(np.abs(sv[m] - s_ref[m][i0:i0 + k]))) / (TOL * max(s_ref[m][0], 1e-300))
        print("zsvd_decomp %s [%d:%d]: shares of bounds 1, 2, 3: %.2e %.2e %.2e" % (A.shape, i0, i0 + k, s1, s2, s3))
        assert max(s1, s2, s3) <= 1.0 and (np.diff(sv[m]) <= 0).all() and (sv[m] >= 0).all()


def check_svd(A):
    U, sv, V = both("zsvd_decomp", A)
    s_ref = np.linalg.svd(A, compute_uv=False)
    check_triplets(A, U, sv, V, s_ref)
    vals = both("zsvd_vals", A)
    assert np.max(np.abs(vals - s_ref)) <= TOL * max(float(np.max(s_ref)), 1e-300)
    return U, sv, V


PHASE = np.array([[1, 2 + 1j], [3 + 4j, 2]], dtype=np.complex128)


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (5, 5), (33, 20), (95, 95), (96, 96), (130, 70), (200, 129), (3, 40, 24)], ids=str)
def test_bidiag_factor(shape):
    check_bidiag(PHASE if shape == (2, 2) else gauss(shape))


@pytest.mark.parametrize("shape", [(1, 1), (7, 7), (95, 95), (96, 96), (150, 60), (100, 70), (60, 150), (300, 300), (4, 33, 33)], ids=str)
def test_svd_decomp(shape):
    check_svd(gauss(shape, 2))


@pytest.mark.parametrize("shape", [(64, 64), (130, 100)], ids=str)
def test_subset(shape):
    A = gauss(shape, 3)
    _, full, _ = both("zsvd_decomp", A)
    U, sv, V = sub("zsvd_decomp", A, (2, 9))
    s_ref = np.linalg.svd(A, compute_uv=False)
    assert sv.shape == (7,) and np.max(np.abs(sv - full[2:9])) <= TOL * s_ref[0]
    check_triplets(A, U, sv, V, s_ref, 2)
    assert np.max(np.abs(sub("zsvd_vals", A, (2, 9)) - full[2:9])) <= TOL * s_ref[0]


def test_special_inputs():
    _, sv, _ = check_svd(gauss((20, 3), 4) @ gauss((3, 20), 5))
    assert (sv[3:] <= TOL * sv[0]).all()
    U, sv, V = both("zsvd_decomp", np.zeros((20, 20), dtype=np.complex128))
    assert not sv.any() and np.isfinite(U).all() and np.isfinite(V).all()
    check_svd(gauss((40, 40), 6) * np.logspace(0, -14, 40))
    _, sv, _ = check_svd(np.linalg.qr(gauss((20, 20), 7))[0])
    assert np.max(np.abs(sv - 1.0)) <= TOL


@pytest.mark.parametrize("shape", [(20, 12), (100, 96)], ids=str)
def test_exact_scaling_and_member_isolation(shape):
    A = gauss(shape, 8)
    stack = np.stack([A, np.ldexp(A.real, 500) + 1j * np.ldexp(A.imag, 500), np.ldexp(A.real, -500) + 1j * np.ldexp(A.imag, -500)])
    one, three = both("zbidiag_factor", A), check_bidiag(stack)
    N = shape[1]
    band = np.eye(shape[0], N, dtype=bool) | np.eye(shape[0], N, 1, dtype=bool)
    su, ss, sv_ = both("zsvd_decomp", A)
    tu, ts, tv = both("zsvd_decomp", stack)
    for m, p in enumerate((0, 500, -500)):
        assert Z.same_bits(np.where(band, 0, three[0][m]), np.where(band, 0, one[0])), "the tails moved"
        assert Z.same_bits(three[1][m], one[1]) and Z.same_bits(three[2][m], one[2])
        assert Z.same_bits(three[3][m], np.ldexp(one[3], p)) and Z.same_bits(three[4][m], np.ldexp(one[4], p))
        assert Z.same_bits(tu[m], su) and Z.same_bits(tv[m], sv_) and Z.same_bits(ts[m], np.ldexp(ss, p))


def test_largest_shape():
    """2048 x 2048 through tier B: |B|_F = |A|_F and bound 1 on 32 fixed rows and columns"""
    n, A = 2048, gauss((2048, 2048), 9)
    F, tauq, taup, d, e = both("zbidiag_factor", A)
    assert abs(np.sqrt(np.sum(d.astype(np.longdouble) ** 2) + np.sum(e.astype(np.longdouble) ** 2)) - fro(A)) <= TOL * fro(A)
    pick = np.arange(32) * 64 + 5
    E = np.zeros((n, 32), dtype=np.complex128)
    E[pick, np.arange(32)] = 1
    B = bidiagonal(d, e)
    cols = both("zqr_apply_q", F, tauq, (B @ both("zbidiag_apply_p", F, taup, E, True).astype(L)).astype(np.complex128))
    rows = both("zbidiag_apply_p", F, taup, (B.T @ both("zqr_apply_q", F, tauq, E, True).astype(L)).astype(np.complex128))
    s_c, s_r = fro(cols - A[:, pick]) / (TOL * fro(A)), fro(rows - H(A[pick, :])) / (TOL * fro(A))
    print("zbidiag_factor 2048 x 2048: shares of bound 1 on 32 columns and rows: %.2e %.2e" % (s_c, s_r))
    assert max(s_c, s_r) <= 1.0


def test_refusals():
    from nd4js_amd import dev
    c = np.complex128
    for fn in (la.zbidiag_factor, la.zsvd_decomp, la.zsvd_vals):
        with pytest.raises(ValueError, match="<= 2048"):
            fn(np.zeros((2049, 2), dtype=c))
    with pytest.raises(ValueError, match="N <= 2048"):
        la.zsvd_decomp(np.zeros((2, 2049), dtype=c))
    with pytest.raises(ValueError, match="M >= N"):
        la.zbidiag_factor(np.zeros((3, 4), dtype=c))
    A = gauss((2, 12, 9), 10)
    before = both("zbidiag_factor", A) + both("zsvd_decomp", A)
    for poison in (np.nan, np.inf):
        Ab = A.copy()
        Ab[1, 3, 4] = poison
        for name, text in (("zbidiag_factor", "zbidiag_factor"), ("zsvd_decomp", "zsvd_decomp"), ("zsvd_vals", "zsvd_decomp")):
            for run in (lambda: getattr(la, name)(Ab), lambda: getattr(dev, name)(_up(Ab))):
                with pytest.raises(_lib.Nd4HipError, match=NOCONV % text) as err:
                    run()
                assert err.value.code == -3
    after = both("zbidiag_factor", A) + both("zsvd_decomp", A)
    assert all(Z.same_bits(x, y) for x, y in zip(before, after))
