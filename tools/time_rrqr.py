"""Device time of the column-pivoted QR family (HIP events around warm calls; every call allocates its own outputs).

    python tools/time_rrqr.py            # the issue's shapes: rrqr_decomp 1024^2, 2048^2, 4096^2, 8192x512, batches
                                         # 1024 x 64^2 and 64 x 512^2, solve 2048^2 with 1 and 2048 right-hand sides
    python tools/time_rrqr.py 2048       # rrqr_decomp of one N x N only
solve = rrqr_decomp + rrqr_lstsq on the device (the host form adds only the rank check on the returned ranks)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms


def main():
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    shapes = [(1, int(n), int(n)) for n in sys.argv[1:]] or [(1, 1024, 1024), (1, 2048, 2048), (1, 4096, 4096), (1, 8192, 512),
                                                             (1024, 64, 64), (64, 512, 512)]
    for b, M, N in shapes:
        A = dev.fill_uniform(7, (b, M, N) if b > 1 else (M, N))
        reps = 3 if M * N >= 4096 * 4096 else 5
        ms, lo, hi = _median_ms(lambda: dev.rrqr_decomp(A), h, reps=reps, warm=1)
        print(json.dumps({"op": "rrqr_decomp", "batch": b, "M": M, "N": N, "median_ms": round(ms, 3), "min_ms": round(lo, 3),
                          "max_ms": round(hi, 3)}), flush=True)
    if len(sys.argv) > 1:
        return
    N = 2048
    A = dev.fill_uniform(7, (N, N))
    for J in (1, 2048):
        Y = dev.fill_uniform(8, (N, J))
        rank = torch.empty((), dtype=torch.int32, device=A.device)

        def solve():
            Q, R, P = dev.rrqr_decomp(A)
            return dev.rrqr_lstsq(Q, R, P, Y, rank=rank)
        ms, lo, hi = _median_ms(solve, h, reps=5, warm=1)
        print(json.dumps({"op": "solve", "N": N, "J": J, "median_ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3)}), flush=True)


if __name__ == "__main__":
    main()
