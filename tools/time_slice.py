"""Times of the strided N-d copy (csrc/gather.hip) behind sliceElems, transpose(...axes), concat and stack: nd4hip_gather_nd_dev on
device-resident operands with the result allocated beforehand and the plan made beforehand (la._*_plan, la._reduce_box), HIP
events around the launches of one operation, median of 10 after 3 warm-ups.

The yardstick is a device-to-device hipMemcpyAsync of as many bytes as the operation writes (so it reads and writes what the
operation reads and writes), on the same stream, in the same run: `ratio` is the operation's time over the copy's. A stepped
inner slice touches more bytes than it keeps (whole 64-byte lines are fetched): `ratio_touched` compares with a copy of half the
bytes touched + written. `ms` is the whole operation between two events, launches included; `kernel_ms` sums
nd4hip_profile_last's kernel time over the operation's launches. Prints one JSON line per case."""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nd4js_amd import _lib, dev, la  # noqa: E402
from time_struct import d2d_copy, timed  # noqa: E402


def launches(dst, dst_off, dst_strides, src, src_off, src_strides, shape):
    """the prepared nd4hip_gather_nd_dev calls of one planned copy"""
    ks, kss, kds, loop = la._reduce_box(shape, src_strides, dst_strides)
    arr = ctypes.c_int64 * max(len(ks), 1)
    h = dev._h(src)
    eb = src.element_size()
    out = []
    for so, do in loop:
        args = (h.ptr, eb, len(ks), arr(*ks), dev._p(src), src.numel(), src_off + so, arr(*kss), dev._p(dst), dst.numel(), dst_off + do, arr(*kds))
        out.append(lambda args=args, keep=(src, dst): _lib.check(h.lib.nd4hip_gather_nd_dev(*args)))     # (keep: the tensors stay alive)
    return out


def slice_case(A, slices):
    shape, off, strides = la._slice_plan(tuple(A.shape), list(slices))
    B = torch.empty(tuple(shape), dtype=A.dtype, device=A.device)
    return B, launches(B, 0, la._c_strides(shape), A, off, strides, shape)


def transpose_case(A, axes):
    shape, strides = la._transpose_plan(tuple(A.shape), axes)
    B = torch.empty(tuple(shape), dtype=A.dtype, device=A.device)
    return B, launches(B, 0, la._c_strides(shape), A, 0, strides, shape)


def list_case(fn, axis, tensors):
    shapes = [list(t.shape) for t in tensors]
    if fn == "concat":
        out_shape, strides, offs = la._concat_plan(axis, shapes)
    else:
        ax, out_shape, strides, offs = la._stack_plan(axis, shapes)
        shapes = [s[:ax] + [1] + s[ax:] for s in shapes]
    B = torch.empty(tuple(out_shape), dtype=tensors[0].dtype, device=tensors[0].device)
    calls = []
    for t, sh, off in zip(tensors, shapes, offs):
        calls += launches(B, off, strides, t, 0, la._c_strides(sh), sh)
    return B, calls


def fill(shape, dtype=torch.float64):
    A = dev.fill_uniform(7, shape)
    return (A * 1e6).to(torch.int32) if dtype == torch.int32 else A


def main(reps=10):
    cases = []
    big = lambda dtype=torch.float64: fill((4096, 4096), dtype)
    cases.append(("A[1:4095, 2:4094]", lambda: slice_case(big(), [(1, 4095), (2, 4094)]), 1.0))
    cases.append(("A[:, :2048]", lambda: slice_case(big(), ["...", (0, 2048)]), 1.0))
    cases.append(("A[::2, :]", lambda: slice_case(big(), [(None, None, 2)]), 1.0))
    cases.append(("A[:, ::2]", lambda: slice_case(big(), ["...", (None, None, 2)]), 1.5))
    cases.append(("A[:, ::-1]", lambda: slice_case(big(), ["...", (None, None, -1)]), 1.0))
    cases.append(("concat(-1, 2 x [4096, 2048])", lambda: list_case("concat", -1, [fill((4096, 2048)), fill((4096, 2048))]), 1.0))
    cases.append(("concat(0, 2 x [2048, 4096])", lambda: list_case("concat", 0, [fill((2048, 4096)), fill((2048, 4096))]), 1.0))
    cases.append(("transpose(2,0,1) of [256, 256, 64]", lambda: transpose_case(fill((256, 256, 64)), (2, 0, 1)), 1.0))
    cases.append(("transpose(1,0,2) of [64, 1024, 64]", lambda: transpose_case(fill((64, 1024, 64)), (1, 0, 2)), 1.0))
    cases.append(("A[7] of [1024, 64, 64]", lambda: slice_case(fill((1024, 64, 64)), [7]), 1.0))
    cases.append(("stack(1, 2 x [1024, 64, 64])", lambda: list_case("stack", 1, [fill((1024, 64, 64)), fill((1024, 64, 64))]), 1.0))
    cases.append(("stack(0, 1024 x [64, 64])", lambda: list_case("stack", 0, list(fill((1024, 64, 64)).unbind(0))), 1.0))
    cases.append(("int32 A[1:4095, 2:4094]", lambda: slice_case(big(torch.int32), [(1, 4095), (2, 4094)]), 1.0))
    cases.append(("int32 A[:, :2048]", lambda: slice_case(big(torch.int32), ["...", (0, 2048)]), 1.0))
    out = []
    for name, make, touched in cases:
        B, calls = make()
        h = dev._h(B)
        nbytes = B.numel() * B.element_size()
        n_copy = max(16, int(nbytes * touched))
        src, dst = torch.empty(n_copy, dtype=torch.uint8, device="cuda"), torch.empty(n_copy, dtype=torch.uint8, device="cuda")
        src.zero_()
        ref = torch.empty(max(16, nbytes), dtype=torch.uint8, device="cuda").zero_()
        ref_dst = torch.empty_like(ref)

        def op():
            for c in calls:
                c()
        copy_ms = timed(lambda: d2d_copy(ref_dst, ref), reps)
        touched_ms = timed(lambda: d2d_copy(dst, src), reps) if touched != 1.0 else copy_ms
        ms = timed(op, reps)
        h.profile_enable(True)
        ks = []
        for _ in range(reps):
            k = 0.0
            for c in calls:
                c()
                k += h.profile_last()[0]["kernel_ms"]
            ks.append(k)
        h.profile_enable(False)
        kernel_ms = sorted(ks)[len(ks) // 2]
        r = {"case": name, "launches": len(calls), "MB_written": round(nbytes / 1e6, 2), "ms": round(ms, 4), "kernel_ms": round(kernel_ms, 4),
             "copy_ms": round(copy_ms, 4), "ratio": round(ms / copy_ms, 2), "kernel_ratio": round(kernel_ms / copy_ms, 2),
             "GB/s": round(2 * nbytes / ms / 1e6, 1), "copy_GB/s": round(2 * nbytes / copy_ms / 1e6, 1)}
        if touched != 1.0:
            r["ratio_touched"] = round(ms / touched_ms, 2)
        out.append(r)
        print(json.dumps(r), flush=True)
        del B, calls, src, dst, ref, ref_dst
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
