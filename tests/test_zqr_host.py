"""zqr_factor / zqr_apply_q / zqr_decomp / zqr_lstsq without a GPU: the model of tests/zqr_common.py inside its bounds and against numpy, the
argument rows of both forms of the C ABI, the argument and dtype errors of la and dev."""
import numpy as np
import pytest

import zqr_common as Q
from nd4js_amd import _lib, la


@pytest.mark.parametrize("shape", Q.LDS_SHAPES + [(5, 40, 24), (300, 4, 4)], ids=Q.name_of)
def test_model_inside_the_bounds_and_against_numpy(shape):
    A = Q.catalogue(*shape)
    assert np.max(np.linalg.cond(A)) <= 1e3
    F, tau = Q.factor_model(A)
    Qm, R = Q.apply_model(F, tau, np.broadcast_to(np.eye(*A.shape[-2:]), A.shape)), np.triu(F[..., :A.shape[-1], :])
    Zm, Y = Q.rhs(A, 3, 5), Q.rhs(A, 3)
    X = Q.lstsq_model(F, tau, Y)
    s1, s2, b3 = Q.shares_qr(A, Qm, R)
    s4 = Q.share_apply(Zm, Q.apply_model(F, tau, Q.apply_model(F, tau, Zm), adjoint=True))
    s5 = Q.share_lstsq(A, X, Y)
    print("%s: model shares of the bounds 1, 2, 4, 5: %.2e %.2e %.2e %.2e" % (Q.name_of(shape), s1, s2, s4, s5))
    assert max(s1, s2, s4, s5) <= 0.1 and b3
    Qn, Rn = np.linalg.qr(A)                                             # both diagonals are real: normalise their signs
    sm, sn = (np.sign(np.diagonal(T, axis1=-2, axis2=-1).real) for T in (R, Rn))
    assert np.allclose(Qm * sm[..., None, :], Qn * sn[..., None, :], rtol=0, atol=1e-10)
    assert np.allclose(R * sm[..., :, None], Rn * sn[..., :, None], rtol=0, atol=1e-10 * np.abs(A).max())
    for m in np.ndindex(A.shape[:-2]):
        assert np.allclose(X[m], np.linalg.lstsq(A[m], Y[m], rcond=None)[0], rtol=0, atol=1e-10)


B = 16           # any non-NULL pointer value
SHAPE, NULL = "the shape must satisfy N <= M <= 2048", "NULL pointer"
ROWS = [  # (operation, the arguments after the handle, the error text after the operation's name or None for an empty call)
    ("zgeqrf_batched", (-1, 4, 3, B, B, B), "negative extent"), ("zgeqrf_batched", (1, 2049, 3, B, B, B), SHAPE),
    ("zgeqrf_batched", (1, 3, 4, B, B, B), SHAPE), ("zgeqrf_batched", (0, 4, 3, B, B, B), None),
    ("zgeqrf_batched", (1, 4, 3, B, B, None), NULL), ("zgeqrf_batched", (1, 4, 3, B, B, B), "NULL handle"),
    ("zungqr_batched", (-1, 4, 3, B, B, B), "negative extent"), ("zungqr_batched", (1, 2049, 3, B, B, B), SHAPE),
    ("zungqr_batched", (1, 3, 4, B, B, B), SHAPE), ("zungqr_batched", (1, 4, 0, B, B, B), None),
    ("zungqr_batched", (1, 4, 3, B, None, B), NULL), ("zungqr_batched", (1, 4, 3, B, B, B), "NULL handle"),
    ("zunmqr_batched", (1, 4, 3, -2, 0, B, 12, B, 3, B), "negative extent"), ("zunmqr_batched", (1, 2049, 3, 2, 0, B, 6147, B, 3, B), SHAPE),
    ("zunmqr_batched", (1, 3, 4, 2, 0, B, 12, B, 4, B), SHAPE), ("zunmqr_batched", (1, 4, 3, 0, 0, B, 12, B, 3, B), None),
    ("zunmqr_batched", (1, 4, 3, 2, 0, B, 12, None, 3, B), NULL), ("zunmqr_batched", (1, 4, 3, 2, 1, B, 0, B, 0, B), "NULL handle"),
    ("zunmqr_batched", (2, 4, 3, 2, 0, B, 12, B, 0, B), "the strides of F and tau must be M*N and N, or both 0"),
    ("zunmqr_batched", (2, 4, 3, 2, 2, B, 12, B, 3, B), "adjoint must be 0 or 1"),
    ("zgels_batched", (-1, 4, 3, 2, B, 12, None, B, B, None), "negative extent"), ("zgels_batched", (1, 2049, 3, 2, B, 6147, None, B, B, None), SHAPE),
    ("zgels_batched", (1, 3, 4, 2, B, 12, None, B, B, None), SHAPE), ("zgels_batched", (0, 4, 3, 2, B, 12, None, B, B, None), None),
    ("zgels_batched", (1, 4, 3, 2, B, 12, None, None, B, None), NULL), ("zgels_batched", (1, 4, 3, 2, B, 0, B, B, B, None), "NULL handle"),
    ("zgels_batched", (2, 4, 3, 2, B, 0, None, B, B, None), "strideA must be M*N, or 0 with a factorisation"),
    ("zgels_batched", (1, 4, 3, 65535 * 64 + 1, B, 12, None, B, B, None), "K exceeds 4 194 240 columns"),
]


@pytest.mark.parametrize("form", ["_host", "_dev"])
def test_both_forms_refuse_alike_before_the_handle(form):
    lib = _lib.load()
    for op, args, text in ROWS:
        rc = getattr(lib, "nd4hip_" + op + form)(None, *args)
        assert (rc, lib.nd4hip_last_error().decode()) == (-1, "nd4hip_%s: %s" % (op, text)) if text else rc == 0, (op, args)


@pytest.fixture
def recorder(monkeypatch):
    """the library must not be reached"""
    monkeypatch.setattr(la._lib, "handle", lambda device=None: pytest.fail("the library was reached"))


def test_an_empty_call_reaches_nothing(recorder):
    c = np.complex128
    F, tau = la.zqr_factor(np.zeros((0, 4, 3), dtype=c))
    assert F.shape == (0, 4, 3) and tau.shape == (0, 3) and la.zqr_factor(np.zeros((2, 3, 0), dtype=c))[1].shape == (2, 0)
    Qe, R = la.zqr_decomp(np.zeros((0, 4, 3), dtype=c))
    assert Qe.shape == (0, 4, 3) and R.shape == (0, 3, 3)
    assert la.zqr_apply_q(np.zeros((4, 3), dtype=c), np.zeros(3, dtype=c), np.zeros((4, 0), dtype=c)).shape == (4, 0)
    info = {}
    assert la.zqr_lstsq(np.zeros((0, 4, 3), dtype=c), np.zeros((0, 4, 2)), info=info).shape == (0, 3, 2) and info["singular"].shape == (0,)


def test_argument_errors(recorder):
    c = np.complex128
    A, tau, Y = np.ones((4, 3), dtype=c), np.zeros(3, dtype=c), np.zeros((4, 2), dtype=c)
    calls = ((la.zqr_factor, "qr_decomp"), (la.zqr_decomp, "qr_decomp"), (lambda a: la.zqr_apply_q(a, tau, Y), "qr_decomp"),
             (lambda a: la.zqr_lstsq(a, Y), "qr_lstsq"), (lambda a: la.zqr_lstsq((a, tau), Y), "qr_lstsq"))
    for fn, real_fn in calls:
        with pytest.raises(TypeError, match=real_fn):
            fn(np.ones((4, 3)))
        with pytest.raises(TypeError, match="only complex128 runs on the GPU path"):
            fn(A.astype(np.complex64))
        for bad, text in ((np.ones((3, 4), dtype=c), "M >= N"), (np.ones(4, dtype=c), "at least 2"), (np.zeros((2049, 1), dtype=c), "M <= 2048")):
            with pytest.raises(ValueError, match=text):
                fn(bad)
    for fn in (lambda y: la.zqr_apply_q(A, tau, y), lambda y: la.zqr_lstsq(A, y), lambda y: la.zqr_lstsq((A, tau), y)):
        with pytest.raises(TypeError, match="complex128 or float64"):
            fn(Y.astype(np.complex64))
        with pytest.raises(ValueError, match="don't match"):
            fn(np.zeros((5, 2), dtype=c))
    for fn in (lambda t: la.zqr_apply_q(A, t, Y), lambda t: la.zqr_lstsq((A, t), Y)):
        with pytest.raises(TypeError, match="tau.dtype must be complex128"):
            fn(np.zeros(3))
    with pytest.raises(ValueError, match="F and tau don't match"):
        la.zqr_apply_q(A, np.zeros(2, dtype=c), Y)
    with pytest.raises(ValueError, match="leading dimensions"):
        la.zqr_apply_q(np.ones((2, 4, 3), dtype=c), np.zeros((2, 3), dtype=c), np.zeros((3, 4, 2), dtype=c))


def test_device_layer_refuses_alike():
    import torch
    from nd4js_amd import dev
    z, r, t = torch.zeros((3, 2), dtype=torch.complex128), torch.zeros((3, 2), dtype=torch.float64), torch.zeros(2, dtype=torch.complex128)
    for fn, real_fn in ((dev.zqr_factor, "qr_decomp"), (dev.zqr_decomp, "qr_decomp"), (lambda a: dev.zqr_apply_q(a, t, z), "qr_decomp"),
                        (lambda a: dev.zqr_lstsq(a, z), "qr_lstsq")):
        with pytest.raises(TypeError, match=real_fn):
            fn(r)
        with pytest.raises(TypeError, match="only complex128"):
            fn(z.to(torch.complex64))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(z)


def test_the_real_family_still_refuses_complex_input():
    z = np.ones((3, 2), dtype=np.complex128)
    for call in (lambda: la.qr_decomp(z), lambda: la.qr_lstsq(z, z, z), lambda: la.lstsq(z, z)):
        with pytest.raises(TypeError, match="complex|must be float"):
            call()
