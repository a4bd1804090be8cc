"""Times of elementwise arithmetic and ordered axis reductions (csrc/elem.hip) behind zip_elems, mapElems and reduceElems:
nd4hip_dzip_nd_dev / nd4hip_dreduce_nd_dev on device-resident operands with the result allocated beforehand and the plan made
beforehand (la._zip_plan, la._reduce_plan), HIP events around the launches of one operation, median of 10 after 3 warm-ups.

The yardstick is a device-to-device hipMemcpyAsync that moves as many bytes as the operation reads plus writes (a copy of n bytes
moves 2 n), on the same stream, in the same run: `ratio` is the operation's time over the copy's. `ms` is the whole operation
between two events, launches included; `kernel_ms` is nd4hip_profile_last's kernel time. The full sum is one dependent chain (the
reference's order is kept): next to it stands what it replaces, a download of the array plus a sequential fold on the host
(numpy's cumsum, which adds in index order). Prints one JSON line per case."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nd4js_amd import _lib, dev, la  # noqa: E402
from time_struct import d2d_copy, timed  # noqa: E402


def zip_case(op, tensors):
    """(result, prepared call, bytes read + written)"""
    shape, _, (bshape, bstrides, loop) = la._zip_plan([tuple(t.shape) for t in tensors])
    C = torch.empty(tuple(shape), dtype=torch.float64, device="cuda")
    nd = len(bshape)
    arr = ctypes.c_int64 * max(nd, 1)
    assert len(loop) == 1
    A, B = tensors[0], tensors[1] if len(tensors) > 1 else None
    h = dev._h(A)
    args = (h.ptr, la.EW_OPS[op], nd, arr(*bshape), dev._p(A), A.numel(), 0, arr(*bstrides[0]), dev._p(B) if B is not None else None,
            B.numel() if B is not None else 0, 0, arr(*bstrides[1]) if B is not None else None, dev._p(C), C.numel())
    moved = 8 * (C.numel() + sum(t.numel() for t in tensors))
    return C, (lambda keep=(tensors, C): _lib.check(h.lib.nd4hip_dzip_nd_dev(*args))), moved


def reduce_case(op, A, axes):
    out_shape, bshape, flags, loop = la._reduce_plan(tuple(A.shape), axes)
    C = torch.empty(tuple(out_shape), dtype=torch.float64, device="cuda")
    nd = len(bshape)
    assert len(loop) == 1
    h = dev._h(A)
    args = (h.ptr, la.EW_OPS[op], nd, (ctypes.c_int64 * max(nd, 1))(*bshape), (ctypes.c_int32 * max(nd, 1))(*flags), dev._p(A), A.numel(),
            dev._p(C), C.numel())
    return C, (lambda keep=(A, C): _lib.check(h.lib.nd4hip_dreduce_nd_dev(*args))), 8 * (A.numel() + C.numel())


def main(reps=10):
    out = []
    # (4096 x 4104: the same work with a row pitch that is no power of two)
    for tag, shape in (("4096^2", (4096, 4096)), ("1024x64^2", (1024, 64, 64)), ("4096x4104", (4096, 4104))):
        A, B = dev.fill_uniform(7, shape), dev.fill_uniform(8, shape)
        col = dev.fill_uniform(9, shape[:-1] + (1,))
        row = dev.fill_uniform(10, (1,) * (len(shape) - 1) + shape[-1:])
        two = torch.full((), 2.5, dtype=torch.float64, device="cuda")
        nd = len(shape)
        cases = [("add(A, B)", lambda: zip_case("add", [A, B])),
                 ("mul(A, scalar)", lambda: zip_case("mul", [A, two])),
                 ("add([..,M,1], [..,1,N])", lambda: zip_case("add", [col, row])),
                 ("neg(A)", lambda: zip_case("neg", [A])),
                 ("sum over the last axis", lambda: reduce_case("add", A, nd - 1)),
                 ("sum over axis %d" % (nd - 2), lambda: reduce_case("add", A, nd - 2)),
                 ("max over the last axis", lambda: reduce_case("max", A, nd - 1)),
                 ("max over every axis", lambda: reduce_case("max", A, list(range(nd)))),
                 ("sum over every axis", lambda: reduce_case("add", A, list(range(nd))))]
        for name, make in cases:
            C, call, moved = make()
            h = dev._h(C)
            n_copy = max(16, moved // 2)
            src = torch.empty(n_copy, dtype=torch.uint8, device="cuda").zero_()
            dst = torch.empty_like(src)
            slow = name == "sum over every axis"
            r_ = 3 if slow else reps
            copy_ms = timed(lambda: d2d_copy(dst, src), reps)
            ms = timed(call, r_, 1 if slow else 3)
            h.profile_enable(True)
            ks = []
            for _ in range(r_):
                call()
                ks.append(h.profile_last()[0]["kernel_ms"])
            h.profile_enable(False)
            kernel_ms = sorted(ks)[len(ks) // 2]
            r = {"case": "%s %s" % (tag, name), "MB_moved": round(moved / 1e6, 2), "ms": round(ms, 4), "kernel_ms": round(kernel_ms, 4),
                 "copy_ms": round(copy_ms, 4), "ratio": round(ms / copy_ms, 2), "kernel_ratio": round(kernel_ms / copy_ms, 2),
                 "GB/s": round(moved / ms / 1e6, 1), "copy_GB/s": round(moved / copy_ms / 1e6, 1)}
            if slow:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x = A.cpu().numpy()
                t1 = time.perf_counter()
                s = np.cumsum(x.reshape(-1))[-1]
                t2 = time.perf_counter()
                r["download_ms"] = round((t1 - t0) * 1e3, 2)
                r["host_fold_ms"] = round((t2 - t1) * 1e3, 2)
                r["same_bits_as_host_fold"] = bool(np.float64(s).view(np.uint64) == C.cpu().numpy().view(np.uint64))
            out.append(r)
            print(json.dumps(r), flush=True)
            del C, call, src, dst
        del A, B, col, row
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
