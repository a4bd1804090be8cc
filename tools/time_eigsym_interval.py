"""Time interval=(lo, hi) beside what it replaces, in one run on device-resident arrays: HIP events, median of 10 after 2 warm-ups (a
call of more than half a second: median of 3). Intervals that hold the 8 largest values and the N / 4 largest values of every member,
their bounds taken from a full eigenvals_sym at midpoints of gaps. Per shape:
  eigen_sym(S, interval) against
    1. eigen_sym(S, subset=(0, k)) with the same k: the difference is the count and its read-back;
    2. what a user does today: the full eigen_sym, the values brought to the host, filtered there, and the columns sliced;
  both reductions; eigenvals_sym likewise (1. only);
  eigen_sym_gen(A, B, interval) and eigen_sym_gen(A, B, subset=(0, 8)) against the full eigen_sym_gen with its columns sliced;
  tridiag_eigen(d, e, interval) at N = 2048 against tridiag_count + tridiag_eigen(subset) as two calls.
Shapes: 1024 x 64^2, 64 x 512^2, 1024^2, 2048^2 (the generalised problem up to 1024^2), each in a child process of its own, as
tools/time_tridiag.py does and for its reason (the workspace arena grows over many calls of changing shapes).
usage: python tools/time_eigsym_interval.py [largest N, default 2048]     all shapes up to that N
       python tools/time_eigsym_interval.py --shape 64x512x512            one shape, in this process ("tridiag": the tridiagonal rows)"""
import os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(1024, 64, 64), (64, 512, 512), (1024, 1024), (2048, 2048)]
GEN_MAX_N = 1024


def _time(fn, h):
    """(median, min, max, reps): the first call decides how many more are affordable"""
    first = _median_ms(fn, h, reps=1, warm=1)[0]
    reps, warm = (10, 2) if first <= 500.0 else (3, 0)
    return _median_ms(fn, h, reps=reps, warm=warm) + (reps,)


T = "median %.2f ms (min %.2f max %.2f, %d runs)"


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        return tridiagonal() if sys.argv[2] == "tridiag" else one(tuple(int(x) for x in sys.argv[2].split("x")))
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    for shape in SHAPES:
        if shape[-1] <= top:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "x".join(str(x) for x in shape)], check=True)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "tridiag"], check=True)


def _bounds(lam, k):
    """(lo [...], +inf): lo the midpoint between the k-th and the (k+1)-th largest value of every member"""
    N = lam.shape[-1]
    lo = 0.5 * (lam[..., k - 1] + lam[..., k]) if k < N else lam[..., N - 1] - 1.0
    return lo.contiguous(), float("inf")


def _filter_today(dev, S, lo):
    """the full spectrum, a filter on the host, the selected columns"""
    L, V = dev.eigen_sym(S)
    keep = (L.cpu() > lo.cpu().unsqueeze(-1)).sum(-1)
    k = int(keep.max())
    return L[..., :k].contiguous(), V[..., :k].contiguous()


def one(shape):
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    A = dev.fill_uniform(7, shape)
    S = (torch.tril(A) + torch.tril(A, -1).transpose(-1, -2)).contiguous()
    N, name = shape[-1], "x".join(str(s) for s in shape)
    lam = dev.eigenvals_sym(S)
    full = _time(lambda: dev.eigen_sym(S), h)
    print("%s: full eigen_sym %s" % (name, T % full), flush=True)
    for k in (8, N // 4):
        lo, hi = _bounds(lam, k)
        info = {}
        dev.eigenvals_sym(S, interval=(lo, hi), info=info)
        kb = (info["range"][..., 1] - info["range"][..., 0]).cpu()
        assert int(kb.min()) == k == int(kb.max()), (k, kb)
        today = _time(lambda: _filter_today(dev, S, lo), h)
        print("%s k = %d: full eigen_sym + host filter + column slice %s" % (name, k, T % today), flush=True)
        for red in (None, "tridiag"):
            iv = _time(lambda: dev.eigen_sym(S, interval=(lo, hi), reduction=red), h)
            sb = _time(lambda: dev.eigen_sym(S, subset=(0, k), reduction=red), h)
            ivv = _time(lambda: dev.eigenvals_sym(S, interval=(lo, hi), reduction=red), h)
            sbv = _time(lambda: dev.eigenvals_sym(S, subset=(0, k), reduction=red), h)
            print("%s k = %d reduction=%s: eigen_sym interval %s  subset %s  interval - subset %.3f ms  interval / today %.2f" %
                  (name, k, red, T % iv, T % sb, iv[0] - sb[0], iv[0] / today[0]), flush=True)
            print("%s k = %d reduction=%s: eigenvals_sym interval %s  subset %s  interval - subset %.3f ms" %
                  (name, k, red, T % ivv, T % sbv, ivv[0] - sbv[0]), flush=True)
    if N > GEN_MAX_N:
        return
    Bm = dev.fill_uniform(11, shape)
    B = (torch.matmul(Bm, Bm.transpose(-1, -2)) / N + torch.eye(N, dtype=torch.float64, device=Bm.device)).contiguous()
    lam = dev.eigenvals_sym_gen(S, B)
    lo, hi = _bounds(lam, 8)
    gfull = _time(lambda: tuple(x[..., :8].contiguous() for x in dev.eigen_sym_gen(S, B)), h)
    gsub = _time(lambda: dev.eigen_sym_gen(S, B, subset=(0, 8)), h)
    giv = _time(lambda: dev.eigen_sym_gen(S, B, interval=(lo, hi)), h)
    gtr = _time(lambda: dev.eigen_sym_gen(S, B, subset=(0, 8), reduction="tridiag"), h)
    print("%s eigen_sym_gen k = 8: full + column slice %s  subset %s = %.2f of it  interval %s = %.2f of it  subset with reduction='tridiag' %s"
          % (name, T % gfull, T % gsub, gsub[0] / gfull[0], T % giv, giv[0] / gfull[0], T % gtr), flush=True)


def tridiagonal():
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    N = 2048
    d, e = dev.fill_uniform(8, (N,)), dev.fill_uniform(9, (N - 1,))
    lam = dev.tridiag_eigenvals(d, e)
    for k in (8, N // 4):
        lo, hi = _bounds(lam, k)
        x = lo.reshape(1).new_tensor([hi, float(lo)])

        def two_calls():
            c = dev.tridiag_count(d, e, x).cpu()
            return dev.tridiag_eigen(d, e, subset=(int(c[0]), int(c[1])))
        assert tuple(two_calls()[0].shape) == (k,)
        iv = _time(lambda: dev.tridiag_eigen(d, e, interval=(lo, hi)), h)
        sb = _time(lambda: dev.tridiag_eigen(d, e, subset=(0, k)), h)
        two = _time(two_calls, h)
        print("tridiag N = %d k = %d: tridiag_eigen interval %s  subset %s  tridiag_count + subset, two calls %s  interval - subset %.3f ms"
              % (N, k, T % iv, T % sb, T % two, iv[0] - sb[0]), flush=True)


if __name__ == "__main__":
    main()
