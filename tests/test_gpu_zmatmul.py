"""GPU parity of complex matmul2 / matmul (matmul2_CC, _CR, _RC of src/la/matmul.js:74-87) through the C ABI, against the
reference's own results in tests/golden/zmatmul (tools/gen_golden_zmatmul.js).

Tolerance as test_gpu_matmul.py: norm-wise relative error <= 1e-13 over the finite entries (1e-10 is the documented gate), and
the NaN / Inf positions (with the sign of each Inf) identical to the reference's, in the real and in the imaginary parts."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from nd4js_amd import _lib, la, rng

pytestmark = pytest.mark.gpu
ZDIR = os.path.join(GOLDEN, "zmatmul")
TIGHT = 1e-13

with open(os.path.join(ZDIR, "manifest.json")) as _f:
    CASES = json.load(_f)["cases"]


def operand(op):
    if "file" in op:
        return np.load(os.path.join(ZDIR, op["file"]))
    n = int(np.prod(op["shape"]))
    if op["dtype"] == "complex128":
        return rng.fill_uniform(op["seed"], 2 * n).view(np.complex128).reshape(op["shape"])
    u = rng.fill_uniform(op["seed"], n).reshape(op["shape"])
    return u if op["dtype"] == "float64" else np.trunc(u * 1000).astype(np.int32)


def case(name):
    meta = CASES[name]
    rows = np.load(os.path.join(ZDIR, meta["rows"])) if "rows" in meta else None
    return operand(meta["A"]), operand(meta["B"]), np.load(os.path.join(ZDIR, meta["C"])), rows


def check_like_reference(got, ref, what):
    assert got.dtype == np.complex128 and got.shape == ref.shape, what
    for part in ("real", "imag"):
        g, r = getattr(got, part), getattr(ref, part)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, part, "NaN positions")
        assert np.array_equal(np.isposinf(g), np.isposinf(r)) and np.array_equal(np.isneginf(g), np.isneginf(r)), (what, part, "Inf positions")
    fin = np.isfinite(ref)
    err = np.linalg.norm((got[fin] - ref[fin]).ravel()) / max(np.linalg.norm(ref[fin].ravel()), 1e-300)
    assert err <= TIGHT, (what, err)


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_host_api(name):
    A, B, ref, rows = case(name)
    C = la.matmul2(A, B)
    check_like_reference(C if rows is None else C[rows], ref, name)


def test_golden_covers_the_contract():
    pairings = {m["pairing"] for m in CASES.values()}
    assert pairings == {"CC", "CR", "RC", "CI", "IC"}
    assert any(m["A"]["shape"][0] >= 1500 and "rows" in m for m in CASES.values())
    assert {"special_CC", "special_CR", "special_RC"} <= set(CASES)
    ref = np.load(os.path.join(ZDIR, CASES["special_CR_inf_only"]["C"]))
    assert np.isinf(ref.real).any() and not np.isnan(ref.imag).any()      # (inf + 0i) * x: no inf * 0 in the CR products


def _dev_shapes(meta):
    """dev.matmul2 takes equal leading axes or one operand without batch; general broadcasting is the host wrapper's job"""
    la_, lb_ = tuple(meta["A"]["shape"][:-2]), tuple(meta["B"]["shape"][:-2])
    return la_ == lb_ or int(np.prod(la_)) == 1 or int(np.prod(lb_)) == 1


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if not n.startswith("large_") and _dev_shapes(CASES[n])])
def test_device_path_bit_identical_to_host_path(name):
    import torch
    from nd4js_amd import dev
    A, B, _, _ = case(name)
    host = la.matmul2(A, B)
    lead_a, lead_b = A.shape[:-2], B.shape[:-2]
    ta = torch.from_numpy(A.astype(np.float64) if A.dtype == np.int32 else A).cuda()
    tb = torch.from_numpy(B.astype(np.float64) if B.dtype == np.int32 else B).cuda()
    got = dev.matmul2(ta.reshape(A.shape[-2:]) if int(np.prod(lead_a)) == 1 and lead_a != lead_b else ta,
                      tb.reshape(B.shape[-2:]) if int(np.prod(lead_b)) == 1 and lead_a != lead_b else tb)
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy().reshape(host.shape), host), name


def test_device_path_at_4096():
    import torch
    from nd4js_amd import dev
    for name in ("large_CC_4096", "large_CR_4096"):
        A, B, ref, rows = case(name)
        host = la.matmul2(A, B)                            # the host form, pipelined over row blocks
        got = dev.matmul2(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()).cpu().numpy()
        assert same_bits(got, host), name
        check_like_reference(got[rows], ref, name)


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n]["pairing"] in ("RC", "IC")])
def test_rc_is_the_real_product_with_the_real_view_of_b(name):
    A, B, _, _ = case(name)
    K, J = B.shape[-2:]
    real = la.matmul2(A, np.ascontiguousarray(B).view(np.float64).reshape(B.shape[:-2] + (K, 2 * J)))
    assert same_bits(la.matmul2(A, B), real.view(np.complex128)), name


def test_empty_and_k0():
    for pa, pb in ((np.complex128, np.complex128), (np.complex128, np.float64), (np.float64, np.complex128)):
        C = la.matmul2(np.ones((3, 0), dtype=pa), np.ones((0, 4), dtype=pb))
        assert C.dtype == np.complex128 and C.shape == (3, 4) and not C.any()
        C = la.matmul2(np.ones((2, 3, 0), dtype=pa), np.ones((0, 5), dtype=pb))
        assert C.shape == (2, 3, 5) and not C.any()
        assert la.matmul2(np.ones((0, 3), dtype=pa), np.ones((3, 4), dtype=pb)).shape == (0, 4)
        assert la.matmul2(np.ones((2, 3), dtype=pa), np.ones((3, 0), dtype=pb)).shape == (2, 0)
    import torch
    from nd4js_amd import dev
    z = dev.matmul2(torch.ones((3, 0), dtype=torch.complex128, device="cuda"), torch.ones((0, 4), dtype=torch.complex128, device="cuda"))
    assert z.shape == (3, 4) and not z.cpu().numpy().any()


def test_out_and_chain():
    A, B, ref, _ = case("pair_CC")
    out = np.full(ref.shape, np.nan, dtype=np.complex128)
    assert la.matmul2(A, B, out=out) is out
    check_like_reference(out, ref, "out=")
    X = rng.fill_uniform(11, 2 * 45 * 3).view(np.complex128).reshape(45, 3)
    Y = rng.fill_uniform(12, 3 * 8).reshape(3, 8)
    got = la.matmul(A, B, X, Y)                            # chain of complex and real operands, ordered by the chain planner
    assert got.dtype == np.complex128
    want = la.matmul2(A, la.matmul2(B, la.matmul2(X, Y)))
    assert np.linalg.norm(got - want) <= TIGHT * np.linalg.norm(want)


def test_multi_device_handle_with_duplicate_ids(monkeypatch):
    monkeypatch.setenv("ND4HIP_TEST_ALLOW_DUP_DEVICES", "1")
    h3 = _lib.Handle([0, 0, 0])
    try:
        A = rng.fill_uniform(8101, 2 * 13 * 40 * 30).view(np.complex128).reshape(13, 40, 30)
        for B in (rng.fill_uniform(8102, 2 * 13 * 30 * 20).view(np.complex128).reshape(13, 30, 20),
                  rng.fill_uniform(8103, 30 * 20).reshape(30, 20)):
            ref = la.matmul2(A, B)
            assert same_bits(la.matmul2(A, B, device=h3), ref)                 # blocks 5 + 4 + 4 on three host threads
            assert same_bits(la.matmul2(A[:2], B[:2] if B.ndim == 3 else B, device=h3), ref[:2])   # spare devices get nothing
        A1, B1, ref1, rows = case("rows_CC_2000")
        check_like_reference(la.matmul2(A1, B1, device=h3)[rows], ref1, "one product on a multi-device handle")
    finally:
        h3.close()


def test_profile_record():
    import torch
    from nd4js_amd import dev
    h = _lib.handle(torch.cuda.current_device())
    A = torch.from_numpy(rng.fill_uniform(8201, 2 * 3 * 70 * 50).view(np.complex128).reshape(3, 70, 50)).cuda()
    B = torch.from_numpy(rng.fill_uniform(8202, 2 * 3 * 50 * 90).view(np.complex128).reshape(3, 50, 90)).cuda()
    R = torch.from_numpy(rng.fill_uniform(8203, 3 * 50 * 90).reshape(3, 50, 90)).cuda()
    h.profile_enable(True)
    try:
        for b, flops in ((B, 8 * 3 * 70 * 50 * 90), (R, 4 * 3 * 70 * 50 * 90)):
            dev.matmul2(A, b)
            torch.cuda.synchronize()
            rec = h.profile_last()[0]
            assert rec["valid"] and rec["op"] == "zgemm_batched" and rec["flops"] == flops and rec["kernel_ms"] > 0, rec
        dev.matmul2(R.transpose(1, 2).contiguous(), B)            # RC: one record, of the complex call, not of the real GEMM inside
        torch.cuda.synchronize()
        rec = h.profile_last()[0]
        assert rec["op"] == "zgemm_batched" and rec["flops"] == 4 * 3 * 90 * 50 * 90, rec
    finally:
        h.profile_enable(False)


def test_device_path_resolves_lazy_conjugates():
    """x.conj() (and a negative view) share the storage of x and only carry a flag: dev.matmul2 must compute with the values
    torch reports, never with the raw storage, and must refuse an `out` whose flag would alter what the kernel writes."""
    import torch
    from nd4js_amd import dev
    A = rng.fill_uniform(8301, 2 * 5 * 7 * 6).view(np.complex128).reshape(5, 7, 6)
    B = rng.fill_uniform(8302, 2 * 5 * 6 * 4).view(np.complex128).reshape(5, 6, 4)
    R = rng.fill_uniform(8303, 5 * 6 * 4).reshape(5, 6, 4)
    ta, tb, tr = (torch.from_numpy(x).cuda() for x in (A, B, R))
    assert ta.conj().is_conj() and ta.conj().is_contiguous() and ta.conj().data_ptr() == ta.data_ptr()
    neg = torch._neg_view(ta)
    assert neg.is_neg()
    for x, y, want in ((ta.conj(), tb, la.matmul2(np.conj(A), B)), (ta, tb.conj(), la.matmul2(A, np.conj(B))),
                       (ta.conj(), tb.conj(), la.matmul2(np.conj(A), np.conj(B))), (ta.conj(), tr, la.matmul2(np.conj(A), R)),
                       (tr.transpose(1, 2).contiguous(), tb.conj(), la.matmul2(np.ascontiguousarray(R.transpose(0, 2, 1)), np.conj(B))),
                       (neg, tb, la.matmul2(-A, B))):
        got = dev.matmul2(x, y)
        torch.cuda.synchronize()
        assert same_bits(got.cpu().numpy(), want)
    out = torch.empty((5, 7, 4), dtype=torch.complex128, device="cuda")
    for bad in (out.conj(), torch._neg_view(out)):
        with pytest.raises(TypeError, match="conjugate or negative"):
            dev.matmul2(ta, tb, out=bad)
    assert dev.matmul2(ta, tb, out=out) is out


@pytest.mark.parametrize("ac,bc", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("shape", [(2, 70, 13, 37), (1, 128, 16, 64)])
def test_unaligned_bases_take_the_scalar_path(ac, bc, shape):
    """Base pointers 8 bytes off a 16-byte boundary (an interleaved buffer at an odd double): the 8-byte load / store variant of
    the kernel (VEC = false; for (1, 128, 16, 64) instead of the unpredicated one), bit for bit what the aligned call gives, and
    nothing written outside C."""
    import ctypes
    import torch
    from nd4js_amd import dev
    batch, I, K, J = shape
    ea, eb = (2 if ac else 1), (2 if bc else 1)
    A = rng.fill_uniform(8401, ea * batch * I * K)
    B = rng.fill_uniform(8402, eb * batch * K * J)
    bufA = torch.zeros(A.size + 1, dtype=torch.float64, device="cuda")
    bufB = torch.zeros(B.size + 1, dtype=torch.float64, device="cuda")
    bufC = torch.full((2 * batch * I * J + 2,), 7.0, dtype=torch.float64, device="cuda")
    bufA[1:].copy_(torch.from_numpy(A))
    bufB[1:].copy_(torch.from_numpy(B))
    h = dev._h(bufC)
    assert (bufA.data_ptr() + 8) % 16 == 8 and (bufC.data_ptr() + 8) % 16 == 8
    _lib.check(h.lib.nd4hip_zgemm_batched_dev(h.ptr, ac, bc, batch, I, K, J, ctypes.c_void_p(bufA.data_ptr() + 8), I * K,
                                              ctypes.c_void_p(bufB.data_ptr() + 8), K * J, ctypes.c_void_p(bufC.data_ptr() + 8)))
    torch.cuda.synchronize()
    c = bufC.cpu().numpy()
    assert c[0] == 7.0 and c[-1] == 7.0
    a = A.view(np.complex128) if ac else A
    b = B.view(np.complex128) if bc else B
    want = la.matmul2(a.reshape(batch, I, K), b.reshape(batch, K, J))
    assert same_bits(c[1:-1].view(np.complex128).reshape(batch, I, J), want)
