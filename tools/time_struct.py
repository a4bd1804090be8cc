"""Times of the structure functions on the device: the _dev entry points on device-resident operands with the result allocated
beforehand, HIP events around each call, median of 10 after 3 warm-ups. Transposition, triu, permute_rows, permute_cols and
unpermute_cols at 4096^2 and at 1024 x 64^2, diag at 4096^2, transposition at 2^20 x 4^2, and permute_rows / permute_cols at
4096 x 4095 (8-byte global accesses on both).

The yardstick is a device-to-device hipMemcpyAsync of as many bytes as the op's result, on the same stream, in the same run: every
op is reported as its time over the copy's (1.0 = as fast as a plain copy, which reads and writes what the op reads and writes).
`ms` is the whole call; the four permutation entry points read one flag word back, so for them it includes that synchronisation.
`kernel_ms` is nd4hip_profile_last's time of the kernels alone. Prints one JSON line per case."""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nd4js_amd import _lib, dev  # noqa: E402

_hip = None


def d2d_copy(dst, src):
    """hipMemcpyAsync(device to device) on torch's current stream"""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        _hip.hipMemcpyAsync.restype = ctypes.c_int
    rc = _hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), 3,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError("hipMemcpyAsync failed with %d" % rc)


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def perm(shape, cols, seed):
    L = shape[-1] if cols else shape[-2]
    g = torch.Generator(device="cpu").manual_seed(seed)
    members = shape[0] if len(shape) > 2 else 1
    P = torch.stack([torch.randperm(L, generator=g) for _ in range(members)])
    return P.reshape(tuple(shape[:-2]) + (L,)).to(torch.int32).cuda()


def main(reps=10):
    out = []
    big, mid, tiny = (4096, 4096), (1024, 64, 64), (1 << 20, 4, 4)
    cases = [(op, s) for s in (big, mid) for op in ("transpose", "triu", "permute_rows", "permute_cols", "unpermute_cols")]
    cases += [("diag", big), ("transpose", tiny)]
    # odd N: the row gather with 8-byte global accesses and no LDS, what separates the two sides of the column gather's time
    cases += [("permute_rows", (4096, 4095)), ("permute_cols", (4096, 4095))]
    for op, shape in cases:
        A = dev.fill_uniform(7, shape)
        M, N = shape[-2:]
        batch = A.numel() // (M * N)
        B = torch.empty(shape[:-1] if op == "diag" else shape, dtype=torch.float64, device="cuda")
        src = torch.empty_like(B) if op == "diag" else A                  # the copy moves what the op writes
        dst = torch.empty_like(src)
        h = dev._h(A)
        lib, p = h.lib, dev._p
        if "permute" in op:
            cols, P = int(op.endswith("cols")), perm(shape, op.endswith("cols"), 11)
            sP = P.shape[-1] if batch > 1 else 0
            fn = lambda: _lib.check(lib.nd4hip_dpermute_batched_dev(h.ptr, cols, int(op.startswith("un")), batch, M, N, p(A),
                                                                    M * N if batch > 1 else 0, p(P), sP, p(B)))
        elif op == "transpose":
            fn = lambda: _lib.check(lib.nd4hip_dtranspose_batched_dev(h.ptr, batch, M, N, p(A), p(B)))
        elif op == "triu":
            fn = lambda: _lib.check(lib.nd4hip_dtri_batched_dev(h.ptr, 1, 0, batch, M, N, p(A), p(B)))
        else:
            fn = lambda: _lib.check(lib.nd4hip_ddiag_batched_dev(h.ptr, batch, M, N, 0, p(A), p(B)))
        copy_ms = timed(lambda: d2d_copy(dst, src), reps)
        ms = timed(fn, reps)
        h.profile_enable(True)
        ks = []
        for _ in range(reps):
            fn()
            ks.append(h.profile_last()[0]["kernel_ms"])
        h.profile_enable(False)
        kernel_ms = sorted(ks)[len(ks) // 2]
        nbytes = 2 * src.numel() * 8
        r = {"op": op, "shape": list(shape), "ms": round(ms, 4), "kernel_ms": round(kernel_ms, 4), "copy_ms": round(copy_ms, 4),
             "ratio_to_copy": round(ms / copy_ms, 2), "kernel_ratio_to_copy": round(kernel_ms / copy_ms, 2),
             "kernel_GB/s": round(nbytes / kernel_ms / 1e6, 1), "copy_GB/s": round(nbytes / copy_ms / 1e6, 1)}
        out.append(r)
        print(json.dumps(r), flush=True)
        del A, B, dst, src
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
