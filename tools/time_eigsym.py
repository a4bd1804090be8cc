"""Time eigen_sym and eigenvals_sym on the device in one run: HIP events, median of 10 after 3 warm-ups, at 512^2, 1024^2, 2048^2,
64 x 512^2 and 1024 x 64^2; `eigen` (the nonsymmetric route) on the same symmetric input where that is affordable (<= 512^2, median
of 3 after 1 warm-up); then the stage split of every shape (nd4hip_dsyevd_last_stages, median of 5).
usage: python tools/time_eigsym.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(512, 512), (1024, 1024), (2048, 2048), (64, 512, 512), (1024, 64, 64)]


def main():
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    for shape in SHAPES:
        A = dev.fill_uniform(7, shape)
        S = torch.tril(A) + torch.tril(A, -1).transpose(-1, -2)
        name = "x".join(str(s) for s in shape)
        full = _median_ms(lambda: dev.eigen_sym(S), h, reps=10, warm=3)
        vals = _median_ms(lambda: dev.eigenvals_sym(S), h, reps=10, warm=3)
        line = "eigen_sym %s median %.2f ms (min %.2f max %.2f)  eigenvals_sym median %.2f ms (min %.2f max %.2f)" % ((name,) + full + vals)
        if len(shape) == 2 and shape[-1] <= 512:
            gen = _median_ms(lambda: dev.eigen(S), h, reps=3, warm=1)
            line += "  eigen median of 3 %.1f ms (min %.1f max %.1f)  eigen/eigen_sym %.0f" % (gen + (gen[0] / full[0],))
        print(line, flush=True)
        h.profile_enable(True)
        try:
            runs = []
            for _ in range(5):
                dev.eigen_sym(S)
                runs.append(h.eigsym_last_stages())
        finally:
            h.profile_enable(False)
        med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}
        print("  stages (ms, median of 5, events between the launches): " + "  ".join("%s %.2f" % kv for kv in med.items())
              + "  sum %.2f" % sum(med.values()), flush=True)


if __name__ == "__main__":
    main()
