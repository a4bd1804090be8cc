"""The structure functions on the device (csrc/struct.hip): transposition, tril / triu, diag / diag_mat and the four permutation
functions, through the host-pointer forms (la.*) and the _dev forms (dev.*), against the reference's recorded results
(tests/golden/struct) and, on shapes that have no fixture, against the numpy restatement of tests/struct_common.py, which
tests/test_struct_host.py holds to every fixture bit for bit.

Nothing is computed, so nothing is approximate: a fixture is met bit for bit (NaN equals NaN, as the reference's copies go
through JS numbers), the restatement in every bit, NaN payloads included. Shapes are the smallest that reach each path: the flat
and the tiled transposition with and without 16-byte accesses (limits STRUCT_FLAT_MAX = 1024 elements, tile 64), member groups,
row blocks, the LDS-staged and the direct column gather, and inverse maps in LDS and in the workspace (STRUCT_LDS_MAP = 4096)."""
import ctypes

import numpy as np
import pytest
import torch

import struct_common as sc
from nd4js_amd import _lib, dev, la

pytestmark = pytest.mark.gpu
ERR_ARG = -1


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both(fn, *args):
    """the result of la.fn (host pointers) and of dev.fn (device tensors), as numpy"""
    host = getattr(la, fn)(*args)
    targs = [to_dev(a) if isinstance(a, np.ndarray) else a for a in args]
    before = [t.clone() if isinstance(t, torch.Tensor) else t for t in targs]
    out = getattr(dev, fn)(*targs)
    torch.cuda.synchronize()
    for t, b in zip(targs, before):                      # inputs are never modified
        if isinstance(t, torch.Tensor):
            assert torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t, b.view(torch.int64) if b.dtype == torch.float64 else b)
    return host, out.cpu().numpy()


def check_exact(fn, *args):
    want = sc.RESTATED[fn](*args)
    for got in both(fn, *args):
        assert got.shape == want.shape, (fn, got.shape, want.shape)
        assert sc.exact_bits(got, want), fn
    return want


# ------------------------------------------------------------------------------------------------ every fixture, both forms
@pytest.mark.parametrize("name", sc.ALL)
def test_fixture_both_forms(name):
    fn, args, want = sc.case(name)
    for got in both(fn, *args):
        assert got.shape == want.shape, name
        assert np.array_equal(np.isnan(got), np.isnan(want)) and sc.same_bits(got, want), name
    check_exact(fn, *args)


# ------------------------------------------------------------------------------------------------ transposition
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (63, 65), (64, 64), (65, 63), (130, 67), (66, 130), (32, 32), (31, 33), (2, 600),
                                   (3, 5, 7), (5, 64, 66), (3, 33, 65)])
def test_transpose_small_shapes(shape):
    want = check_exact("transpose", sc.special(1, *shape))
    assert want.shape == shape[:-2] + (shape[-1], shape[-2])


def test_transpose_seventy_thousand_members_take_the_flat_form():
    A = sc.special(2, 70000, 3, 5)
    check_exact("transpose", A)


@pytest.mark.parametrize("shape", [(2049, 2047), (2048, 2048)])
def test_transpose_large(shape):
    A = sc.special(3, *shape)
    check_exact("transpose", A)


def test_transpose_of_a_misaligned_view_takes_the_8_byte_path():
    base = to_dev(sc.special(4, 64 * 66 + 1))
    A = base[1:].view(64, 66)                            # even sizes, base address only 8-byte aligned
    assert A.data_ptr() % 16 == 8
    B = dev.transpose(A)
    assert sc.exact_bits(B.cpu().numpy(), sc.transpose(A.cpu().numpy()))
    assert sc.exact_bits(dev.transpose(B).cpu().numpy(), A.cpu().numpy())
    assert sc.exact_bits(dev.triu(A, 1).cpu().numpy(), sc.triu(A.cpu().numpy(), 1))
    P = to_dev(sc.index_vector("perm", 5, (), 64))
    assert sc.exact_bits(dev.permute_rows(A, P).cpu().numpy(), sc.permute_rows(A.cpu().numpy(), P.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ tril / triu
@pytest.mark.parametrize("fn", ["tril", "triu"])
def test_tri_offsets(fn):
    for shape in [(5, 8), (8, 5)]:
        A = sc.special(6, *shape)
        for k in (-9, -5, -1, 0, 1, 5, 9, -2 ** 63, 2 ** 63 - 1):
            check_exact(fn, A, k)
    A = sc.special(7, 130, 67)
    A[3, 0] = A[0, 3] = A[4, 1] = np.nan
    A[2, 5] = A[5, 2] = -0.0
    for k in (-3, 3):
        check_exact(fn, A, k)
    check_exact(fn, sc.special(8, 3, 9, 6), 1)           # even N: the 16-byte form over a batch
    check_exact(fn, sc.special(9, 70000, 3, 5), -1)


# ------------------------------------------------------------------------------------------------ diag / diag_mat
def test_diag_every_offset_and_its_neighbours():
    for M, N in [(5, 8), (8, 5)]:
        A = sc.special(10, 2, M, N)
        for off in range(-M + 1, N):
            want = check_exact("diag", A, off)
            assert want.shape == (2, min(M, M + off, N, N - off))
        for off in (-M, N):
            for mod, arg in ((la, A), (dev, to_dev(A))):
                with pytest.raises(ValueError) as info:
                    mod.diag(arg, off)
                assert str(info.value) == "diag(A, offset): offset=%d out of A.shape=[undefined]." % off
        h = _lib.handle()
        d = np.empty((2, 8))
        assert h.lib.nd4hip_ddiag_batched(h.ptr, 2, M, N, N, la._ptr(A), la._ptr(d)) == ERR_ARG
    check_exact("diag", sc.special(11, 4096 + 3, 7), 0)


@pytest.mark.parametrize("shape", [(7,), (3, 1), (2, 3, 65), (5, 66), (70000, 3)])
def test_diag_mat(shape):
    d = sc.special(12, *shape)
    host = np.full(shape + (shape[-1],), 7.0)            # D is written completely, zeros included
    h = _lib.handle()
    _lib.check(h.lib.nd4hip_ddiagmat_batched(h.ptr, int(np.prod(shape[:-1], dtype=np.int64)), shape[-1], la._ptr(d), la._ptr(host)))
    assert sc.exact_bits(host, sc.diag_mat(d))
    check_exact("diag_mat", d)


# ------------------------------------------------------------------------------------------------ the four permutation functions
@pytest.mark.parametrize("fn", sc.PERM)
@pytest.mark.parametrize("kind", ["perm", "identity", "dup"])
def test_permutations_on_every_path(fn, kind):
    cols = fn.endswith("cols")
    shapes = [((1, 1), ()), ((33, 1), ()), ((1, 33), ()), ((65, 130), ()), ((65, 131), ()),      # odd N: 8-byte rows
              ((9, 6), (3,)), ((3, 9, 6), (1,)), ((2, 1, 9, 6), (3,)),                           # the broadcast rules
              ((3, 100, 70), (3,)),                                                                 # row blocks of a batch
              ((4100, 3), ()) if not cols else ((2, 4100), ())]                                     # an inverse map beyond LDS
    for a_shape, p_lead in shapes:
        L = a_shape[-1] if cols else a_shape[-2]
        A, P = sc.special(13, *a_shape), sc.index_vector(kind, 14, p_lead, L)
        want = check_exact(fn, A, P)
        assert want.ndim == max(A.ndim, P.ndim + 1)
        if kind == "dup" and fn.startswith("un") and L >= 33:
            p = P.reshape(-1, L)[0]
            missing = np.setdiff1d(np.arange(L), p)
            assert missing.size and np.unique(p).size < L
            first = want.reshape((-1,) + want.shape[-2:])[0]
            gone = first[:, missing] if cols else first[missing, :]
            assert not sc.bits(gone).any()                                                          # +0.0, every bit
            k = p[-1]                                                                               # the last writer
            src = A.reshape((-1,) + A.shape[-2:])[0]
            assert sc.exact_bits(first[:, k] if cols else first[k, :], src[:, L - 1] if cols else src[L - 1, :])


@pytest.mark.parametrize("fn", sc.PERM)
def test_permutations_of_seventy_thousand_members(fn):
    cols = fn.endswith("cols")
    A = sc.special(15, 70000, 3, 5)
    P = sc.index_vector("dup", 16, (70000,), 5 if cols else 3)
    check_exact(fn, A, P)


@pytest.mark.parametrize("fn", sc.PERM)
def test_permutations_are_deterministic(fn):
    cols = fn.endswith("cols")
    A, P = to_dev(sc.special(17, 4, 200, 300)), to_dev(sc.index_vector("dup", 18, (4,), 300 if cols else 200))
    first = getattr(dev, fn)(A, P)
    for _ in range(3):
        assert torch.equal(getattr(dev, fn)(A, P).view(torch.int64), first.view(torch.int64))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("i", [i for i, e in enumerate(sc.ERRORS) if e.get("on_device")])
def test_index_out_of_range_is_an_error_and_the_handle_stays_usable(i):
    e = sc.ERRORS[i]
    fn = e["fn"]
    cols, inverse = int(fn.endswith("cols")), int(fn.startswith("un"))
    _, P = sc.refused_call(e)
    A = sc.special(19, *e["a_shape"])
    batch, M, N = A.shape
    L = P.shape[-1]
    h = _lib.handle()
    # host-pointer form, raw: the code and the recorded text
    B = np.empty_like(A)
    rc = h.lib.nd4hip_dpermute_batched(h.ptr, cols, inverse, batch, M, N, la._ptr(A), M * N, la._ptr(P), L, la._ptr(B))
    assert rc == ERR_ARG and h.lib.nd4hip_last_error().decode() == e["message"]
    # the _dev form, raw
    tA, tP, tB = to_dev(A), to_dev(P), torch.empty(A.shape, dtype=torch.float64, device="cuda")
    hd = dev._h(tA)
    rc = h.lib.nd4hip_dpermute_batched_dev(hd.ptr, cols, inverse, batch, M, N, dev._p(tA), M * N, dev._p(tP), L, dev._p(tB))
    assert rc == ERR_ARG and h.lib.nd4hip_last_error().decode() == e["message"]
    # the wrappers raise it as the reference's text
    for mod, a, p in ((la, A, P), (dev, tA, tP)):
        with pytest.raises(ValueError) as info:
            getattr(mod, fn)(a, p)
        assert str(info.value) == e["message"]
    # a following valid call processes the other members: the handle is usable
    good = np.ascontiguousarray(P[[0, 2]])
    check_exact(fn, np.ascontiguousarray(A[[0, 2]]), good)


def test_overlapping_output_is_refused():
    h = _lib.handle()
    buf = np.zeros(2 * 6 * 6 + 8)
    P = np.arange(6, dtype=np.int32)
    t, tP = to_dev(buf), to_dev(P)
    hd = dev._h(t)
    lib = h.lib
    # (host form, _dev form, offset of the input, offset of the output) in doubles: the two spans share elements
    calls = [
        (lambda f, hp_, a, b, pp: f(hp_, 1, 6, 6, a, b), lib.nd4hip_dtranspose_batched, lib.nd4hip_dtranspose_batched_dev, 0, 8),
        (lambda f, hp_, a, b, pp: f(hp_, 1, 0, 1, 6, 6, a, b), lib.nd4hip_dtri_batched, lib.nd4hip_dtri_batched_dev, 0, 8),
        (lambda f, hp_, a, b, pp: f(hp_, 1, 6, 6, 0, a, b), lib.nd4hip_ddiag_batched, lib.nd4hip_ddiag_batched_dev, 0, 8),
        (lambda f, hp_, a, b, pp: f(hp_, 1, 6, a, b), lib.nd4hip_ddiagmat_batched, lib.nd4hip_ddiagmat_batched_dev, 10, 8),
        (lambda f, hp_, a, b, pp: f(hp_, 0, 0, 1, 6, 6, a, 0, pp, 0, b), lib.nd4hip_dpermute_batched, lib.nd4hip_dpermute_batched_dev, 0, 8),
        (lambda f, hp_, a, b, pp: f(hp_, 1, 1, 1, 6, 6, a, 0, pp, 0, b), lib.nd4hip_dpermute_batched, lib.nd4hip_dpermute_batched_dev, 35, 0),
    ]
    for call, host_fn, dev_fn, oa, ob in calls:
        hp = lambda off: ctypes.c_void_p(buf.ctypes.data + 8 * off)
        dp = lambda off: ctypes.c_void_p(t.data_ptr() + 8 * off)
        for b_off in (ob, oa):                                       # partly overlapping, and in place
            assert call(host_fn, h.ptr, hp(oa), hp(b_off), la._ptr(P)) == ERR_ARG
            assert "overlap" in lib.nd4hip_last_error().decode()
            assert call(dev_fn, hd.ptr, dp(oa), dp(b_off), dev._p(tP)) == ERR_ARG
            assert "overlap" in lib.nd4hip_last_error().decode()
    assert not buf.any() and not t.cpu().numpy().any()               # nothing was written


def test_profile_reports_bytes_and_no_flops():
    A = to_dev(sc.special(20, 4, 64, 66))
    h = dev._h(A)
    h.profile_enable(True)
    try:
        dev.transpose(A)
        rec = h.profile_last()[0]
        assert rec["valid"] and rec["op"] == "dtranspose_batched" and rec["flops"] == 0.0 and rec["bytes"] == 16.0 * A.numel()
        dev.permute_cols(A, to_dev(sc.index_vector("perm", 1, (), 66)))
        rec = h.profile_last()[0]
        assert rec["valid"] and rec["op"] == "dpermute_batched" and rec["flops"] == 0.0 and rec["bytes"] == 16.0 * A.numel() + 4 * 66
    finally:
        h.profile_enable(False)


def test_host_forms_shard_over_the_devices_of_a_handle(monkeypatch):
    """blocks 5 + 4 + 4 of a batch of 13 on three host threads (the same device three times); broadcast operands go to every block"""
    monkeypatch.setenv("ND4HIP_TEST_ALLOW_DUP_DEVICES", "1")
    h3 = _lib.Handle([0, 0, 0])
    try:
        A, d = sc.special(22, 13, 9, 6), sc.special(23, 13, 7)
        assert sc.exact_bits(la.transpose(A, device=h3), sc.transpose(A))
        assert sc.exact_bits(la.triu(A, 1, device=h3), sc.triu(A, 1))
        assert sc.exact_bits(la.diag(A, -2, device=h3), sc.diag(A, -2))
        assert sc.exact_bits(la.diag_mat(d, device=h3), sc.diag_mat(d))
        for fn in sc.PERM:
            L = 6 if fn.endswith("cols") else 9
            for P in (sc.index_vector("dup", 24, (13,), L), sc.index_vector("perm", 25, (), L)):
                assert sc.exact_bits(getattr(la, fn)(A, P, device=h3), sc.RESTATED[fn](A, P)), fn
            bad = sc.index_vector("perm", 26, (13,), L)
            bad[11, 2] = L                                        # in the last block: reported with its device, the handle stays usable
            with pytest.raises(ValueError, match=r"%s\(A,P\): P\.contains invalid indices\." % fn):
                getattr(la, fn)(A, bad, device=h3)
            assert sc.exact_bits(getattr(la, fn)(A[:2], bad[:2], device=h3), sc.RESTATED[fn](A[:2], bad[:2]))
    finally:
        h3.close()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ one chain that stays on the device
def test_lu_chain_on_device_arrays_only():
    """P A = L U with every step on device tensors: permute_rows(A, P) against matmul2(tril(LU, -1) + I, triu(LU))"""
    N = 96
    A_host = np.random.default_rng(21).uniform(-1.0, 1.0, size=(3, N, N))
    A = to_dev(A_host)
    LU, P = dev.lu_decomp(A)
    Lm = dev.tril(LU, -1) + dev.diag_mat(torch.ones(3, N, dtype=torch.float64, device="cuda"))
    PA = dev.permute_rows(A, P)
    LUprod = dev.matmul2(Lm, dev.triu(LU))
    assert all(t.is_cuda for t in (LU, P, Lm, PA, LUprod))
    # the host result: the same chain through la.*
    LUh, Ph = la.lu_decomp(A_host)
    PAh = la.permute_rows(A_host, Ph)
    Lh = la.tril(LUh, -1) + la.diag_mat(np.ones((3, N)))
    prod_h = la.matmul2(Lh, la.triu(LUh))
    scale = np.linalg.norm(PAh)
    assert sc.exact_bits(PA.cpu().numpy(), PAh)
    assert np.linalg.norm(LUprod.cpu().numpy() - prod_h) <= sc.GATE * scale
    assert np.linalg.norm(LUprod.cpu().numpy() - PA.cpu().numpy()) <= sc.GATE * scale
    d = dev.diag(LU)                                           # 3 x N doubles instead of 3 x N x N to read the pivots
    assert sc.exact_bits(d.cpu().numpy(), np.diagonal(LUh, axis1=-2, axis2=-1))
