"""Time the symmetric tridiagonal reduction beside what it replaces, in one run on device-resident arrays: HIP events, median of 10
after 2 warm-ups (a call of more than half a second: median of 3).
  tridiag_factor, tridiag_decomp and hessenberg_decomp (of the symmetrised member);
  eigen_sym / eigenvals_sym with and without reduction='tridiag', with subset=(0, 8) and with no subset, each with its stage times
  (nd4hip_dsyevd_last_stages / nd4hip_dsyevx_last_stages: median of the same number of runs, and the smallest and largest of the
  reduce stage, which is what the keyword changes).
Shapes: 1024 x 64^2, 256 x 128^2, 64 x 512^2, 4 x 1024^2, 512^2, 1024^2, 2048^2, each in a child process of its own: the handle's
workspace arena keeps growing over hundreds of eigen_sym calls of changing shapes (the default route's as well), and one process for
all of them runs out of device memory.
usage: python tools/time_tridiag.py [largest N, default 2048]     all shapes up to that N
       python tools/time_tridiag.py --shape 64x512x512            one shape, in this process"""
import os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(1024, 64, 64), (256, 128, 128), (64, 512, 512), (4, 1024, 1024), (512, 512), (1024, 1024), (2048, 2048)]


def _time(fn, h):
    """(median, min, max, reps): the first call decides how many more are affordable"""
    first = _median_ms(fn, h, reps=1, warm=1)[0]
    reps, warm = (10, 2) if first <= 500.0 else (3, 0)
    return _median_ms(fn, h, reps=reps, warm=warm) + (reps,)


def _stages(fn, h, read, reps):
    """the per-stage medians as text, and (median, min, max) of the reduce stage"""
    h.profile_enable(True)
    try:
        fn()
        runs = []
        for _ in range(reps):
            fn()
            runs.append(read())
    finally:
        h.profile_enable(False)
    med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}
    red = sorted(r["reduce"] for r in runs)
    return "  ".join("%s %.2f" % kv for kv in med.items()) + "  sum %.2f" % sum(med.values()), (med["reduce"], red[0], red[-1])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        return one(tuple(int(x) for x in sys.argv[2].split("x")))
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    for shape in SHAPES:
        if shape[-1] <= top:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "x".join(str(x) for x in shape)], check=True)


def one(shape):
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    A = dev.fill_uniform(7, shape)
    S = (torch.tril(A) + torch.tril(A, -1).transpose(-1, -2)).contiguous()
    N, name = shape[-1], "x".join(str(s) for s in shape)
    f = _time(lambda: dev.tridiag_factor(S), h)
    q = _time(lambda: dev.tridiag_decomp(S), h)
    g = _time(lambda: dev.hessenberg_decomp(S), h)
    print("%s: tridiag_factor median %.2f ms (min %.2f max %.2f, %d runs)  tridiag_decomp %.2f ms (min %.2f max %.2f, %d runs)  "
          "hessenberg_decomp %.2f ms (min %.2f max %.2f, %d runs)" % ((name,) + f + q + g), flush=True)
    for sub in ((0, 8), None):
        kw = {} if sub is None else {"subset": sub}
        read = h.eigsym_last_stages if sub is None else h.eigsym_subset_last_stages
        rows = {}
        for red in (None, "tridiag"):
            full = _time(lambda: dev.eigen_sym(S, reduction=red, **kw), h)
            vals = _time(lambda: dev.eigenvals_sym(S, reduction=red, **kw), h)
            text, reduce = _stages(lambda: dev.eigen_sym(S, reduction=red, **kw), h, read, full[3])
            rows[red] = (full, vals, reduce)
            print("%s subset=%s reduction=%s: eigen_sym median %.2f ms (min %.2f max %.2f, %d runs)  eigenvals_sym median %.2f ms (min %.2f "
                  "max %.2f, %d runs)" % ((name, sub, red) + full + vals), flush=True)
            print("  stages of eigen_sym (ms, median): " + text + "   reduce: median %.2f min %.2f max %.2f" % reduce, flush=True)
        d, t = rows[None], rows["tridiag"]
        print("  reduction='tridiag' / default: eigen_sym %.2f  eigenvals_sym %.2f  reduce stage %.2f; its median %s the default's smallest run"
              % (t[0][0] / d[0][0], t[1][0] / d[1][0], t[2][0] / d[2][0], "lies below" if t[2][0] < d[2][1] else "does NOT lie below"), flush=True)


if __name__ == "__main__":
    main()
