"""Device time of the strong rank-revealing QR (HIP events around warm calls; every call allocates its own outputs).

    python tools/time_srrqr.py           # srrqr_decomp_full 512^2, 1024^2, 2048^2 and the batches 1024 x 64^2, 64 x 512^2;
                                         # urv_decomp_full 1024^2; urv_lstsq 2048^2 with 2048 right-hand sides
    python tools/time_srrqr.py 1024      # one N x N only
Each call is the decision pass (one workgroup per matrix) plus the full QR of A[:, P]."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms


def main():
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    shapes = [(1, int(n), int(n)) for n in sys.argv[1:]] or [(1, 512, 512), (1, 1024, 1024), (1, 2048, 2048), (1024, 64, 64),
                                                             (64, 512, 512)]
    for b, M, N in shapes:
        A = dev.fill_uniform(7, (b, M, N) if b > 1 else (M, N))
        reps = 3 if M * N >= 2048 * 2048 else 5
        ms, lo, hi = _median_ms(lambda: dev.srrqr_decomp_full(A), h, reps=reps, warm=1)
        r = dev.srrqr_decomp_full(A)[3]
        print(json.dumps({"op": "srrqr_decomp_full", "batch": b, "M": M, "N": N, "median_ms": round(ms, 3), "min_ms": round(lo, 3),
                          "max_ms": round(hi, 3), "rank_min": int(r.min())}), flush=True)
    if len(sys.argv) > 1:
        return
    A = dev.fill_uniform(7, (1024, 1024))
    ms, lo, hi = _median_ms(lambda: dev.urv_decomp_full(A), h, reps=3, warm=1)
    print(json.dumps({"op": "urv_decomp_full", "M": 1024, "N": 1024, "median_ms": round(ms, 3), "min_ms": round(lo, 3),
                      "max_ms": round(hi, 3)}), flush=True)
    N = 2048
    A = dev.fill_uniform(7, (N, N))
    U, R, V, r = dev.urv_decomp_full(A)
    Y = dev.fill_uniform(8, (N, N))
    ms, lo, hi = _median_ms(lambda: dev.urv_lstsq(U, R, V, r, Y), h, reps=5, warm=1)
    print(json.dumps({"op": "urv_lstsq", "N": N, "J": N, "median_ms": round(ms, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3)}),
          flush=True)


if __name__ == "__main__":
    main()
