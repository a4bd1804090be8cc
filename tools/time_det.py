"""Times of det / slogdet / norm on the device (device-resident inputs, HIP events around the _dev entry points):
2^20 x 4x4 det, 10^4 x 32^2 and 1024 x 64^2 det, slogdet 2048^2 (with qr_decomp 2048^2 for comparison), the R-only QR at 4096^2
(slogdet 4096^2), norm 4096^2. Prints one JSON line per case: median of `reps` runs after one warm-up."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nd4js_amd import dev  # noqa: E402


def timed(fn, reps):
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


def main(reps=10):
    out = []
    cases = [("det", (1 << 20, 4, 4)), ("det", (10000, 32, 32)), ("det", (1024, 64, 64)), ("slogdet", (2048, 2048)),
             ("qr_decomp", (2048, 2048)), ("slogdet", (4096, 4096)), ("norm", (4096, 4096))]
    for op, shape in cases:
        A = dev.fill_uniform(7, shape)
        fn = {"det": lambda: dev.det(A), "slogdet": lambda: dev.slogdet(A), "qr_decomp": lambda: dev.qr_decomp(A),
              "norm": lambda: dev.norm(A)}[op]
        ms = timed(fn, reps if shape[-1] < 4096 else 3)
        r = {"op": op, "shape": list(shape), "ms": round(ms, 4)}
        if op in ("norm", "det") and shape[-1] <= 4096:
            r["GB/s"] = round(A.numel() * 8 / ms / 1e6, 1)
        out.append(r)
        print(json.dumps(r), flush=True)
        del A
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
