"""Time eigen_sym / eigenvals_sym with subset=(0, 8) and subset=(0, N) beside the unchanged default route in one run: HIP events,
median of 10 after 3 warm-ups (a call that takes more than half a second: median of 3 after 1), at 512^2, 1024^2, 2048^2, 64 x 512^2
and 1024 x 64^2; the stage split of the subset calls (nd4hip_dsyevx_last_stages, median of 5, or of 3); then tridiag_eigen alone at
N = 2048, k = 8 and k = 2048.
usage: python tools/time_eigsym_subset.py [largest N, default 2048]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(512, 512), (1024, 1024), (2048, 2048), (64, 512, 512), (1024, 64, 64)]


def _time(fn, h):
    """(median, min, max, reps): the first call decides how many more are affordable"""
    first = _median_ms(fn, h, reps=1, warm=1)[0]
    reps, warm = (10, 2) if first <= 500.0 else (3, 0)
    return _median_ms(fn, h, reps=reps, warm=warm) + (reps,)


def _stages(fn, h, read, reps):
    h.profile_enable(True)
    try:
        runs = []
        for _ in range(reps):
            fn()
            runs.append(read())
    finally:
        h.profile_enable(False)
    med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}
    return "  ".join("%s %.2f" % kv for kv in med.items()) + "  sum %.2f" % sum(med.values())


def main():
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    for shape in SHAPES:
        if shape[-1] > top:
            continue
        A = dev.fill_uniform(7, shape)
        S = torch.tril(A) + torch.tril(A, -1).transpose(-1, -2)
        N, name = shape[-1], "x".join(str(s) for s in shape)
        full = _time(lambda: dev.eigen_sym(S), h)
        vals = _time(lambda: dev.eigenvals_sym(S), h)
        print("%s default route: eigen_sym median %.2f ms (min %.2f max %.2f, %d runs)  eigenvals_sym median %.2f ms (min %.2f max %.2f, %d runs)"
              % ((name,) + full + vals), flush=True)
        for sub in ((0, 8), (0, N)):
            f = _time(lambda: dev.eigen_sym(S, subset=sub), h)
            v = _time(lambda: dev.eigenvals_sym(S, subset=sub), h)
            print("%s subset=%s: eigen_sym median %.2f ms (min %.2f max %.2f, %d runs) = %.2f of the default  eigenvals_sym median %.2f ms "
                  "(min %.2f max %.2f, %d runs) = %.2f of the default" % ((name, sub) + f + (f[0] / full[0],) + v + (v[0] / vals[0],)), flush=True)
            print("  stages of eigen_sym (ms, median, events between the launches): "
                  + _stages(lambda: dev.eigen_sym(S, subset=sub), h, h.eigsym_subset_last_stages, 5 if f[0] <= 500.0 else 3), flush=True)
    N = min(top, 2048)
    d, e = dev.fill_uniform(8, (N,)), dev.fill_uniform(9, (N - 1,))
    for k in (8, N):
        f = _time(lambda: dev.tridiag_eigen(d, e, subset=(0, k)), h)
        v = _time(lambda: dev.tridiag_eigenvals(d, e, subset=(0, k)), h)
        print("tridiag N = %d k = %d: tridiag_eigen median %.2f ms (min %.2f max %.2f, %d runs)  tridiag_eigenvals median %.2f ms (min %.2f max %.2f, "
              "%d runs)" % ((N, k) + f + v), flush=True)
        print("  stages of tridiag_eigen: " + _stages(lambda: dev.tridiag_eigen(d, e, subset=(0, k)), h, h.eigsym_subset_last_stages, 3), flush=True)


if __name__ == "__main__":
    main()
