"""Time svd_decomp(A, algo='dc') against algo='jacobi' on the device in one run: HIP events, median of 10 after 3 warm-ups,
at 512^2, 1024^2, 2048^2 and 64 x 512^2, then the per-stage split of the 2048^2 divide & conquer run (nd4hip_dgesdd_last_stages).
usage: python tools/time_svd_dc.py [N ...]      (sizes of single matrices; the batch 64 x 512^2 always runs)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms


def main():
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    sizes = [(N, N) for N in [int(x) for x in sys.argv[1:]] or [512, 1024, 2048]] + [(64, 512, 512)]
    for shape in sizes:
        A = dev.fill_uniform(7, shape)
        row = {}
        for algo in ("dc", "jacobi"):
            row[algo] = _median_ms(lambda: dev.svd_decomp(A, algo=algo), h, reps=10, warm=3)
        print("svd_decomp %s  dc median %.2f ms (min %.2f max %.2f)  jacobi median %.2f ms (min %.2f max %.2f)  dc/jacobi %.2f"
              % ("x".join(str(s) for s in shape), *row["dc"], *row["jacobi"], row["dc"][0] / row["jacobi"][0]), flush=True)
    N = sizes[-2][0]
    A = dev.fill_uniform(7, (N, N))
    h.profile_enable(True)
    try:
        runs = []
        for _ in range(5):
            dev.svd_decomp(A, algo="dc")
            runs.append(h.svd_dc_last_stages())
    finally:
        h.profile_enable(False)
    med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}
    print("stages of dc at %d^2 (ms, median of 5, events between the launches): " % N
          + "  ".join("%s %.2f" % kv for kv in med.items()) + "  sum %.2f" % sum(med.values()), flush=True)


if __name__ == "__main__":
    main()
