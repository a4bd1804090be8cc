"""Time the Hermitian eigenproblem beside what a user had before it, in one run: HIP events on device-resident arrays, median of 10
after 2 warm-ups (a call of more than half a second: median of 3).
  herm_tridiag_factor, eigen_herm and eigenvals_herm, full and with subset=(0, 8);
  the real embedding [[A, -B], [B, A]] of order 2 N (where 2 N <= 2048) through eigen_sym(reduction='tridiag') and the default eigen_sym;
  numpy.linalg.eigh of the same matrices on the host (wall clock, one run).
Shapes: 1024 x 64^2, 64 x 512^2, 512^2, 1024^2, 2048^2, each in a child process of its own (the handle's workspace arena keeps growing
over many calls of changing shapes). Every line ends with the ratio eigen_herm / the other; above 1 the Hermitian route loses.
usage: python tools/time_eigherm.py [largest N, default 2048]     all shapes up to that N
       python tools/time_eigherm.py --shape 64x512x512            one shape, in this process"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(1024, 64, 64), (64, 512, 512), (512, 512), (1024, 1024), (2048, 2048)]


def _time(fn, h):
    """(median, min, max, reps): the first call decides how many more are affordable"""
    first = _median_ms(fn, h, reps=1, warm=1)[0]
    reps, warm = (10, 2) if first <= 500.0 else (3, 0)
    return _median_ms(fn, h, reps=reps, warm=warm) + (reps,)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        return one(tuple(int(x) for x in sys.argv[2].split("x")), "--embedding" in sys.argv)
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    for shape in SHAPES:
        if shape[-1] <= top:
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", "x".join(str(x) for x in shape)]
            subprocess.run(cmd, check=True)
            # the embedding in a process of its own: eigen_sym's workspace for 64 x 1024^2 alone is most of the device's memory
            if 2 * shape[-1] <= 2048 and subprocess.run(cmd + ["--embedding"]).returncode != 0:
                print("%s: the embedding of order %d did not finish (see above)" % (cmd[-1], 2 * shape[-1]), flush=True)


def one(shape, embedding=False):
    import numpy as np
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    A, B = dev.fill_uniform(7, shape), dev.fill_uniform(8, shape)
    A = (torch.tril(A) + torch.tril(A, -1).transpose(-1, -2)).contiguous()
    B = (torch.tril(B, -1) - torch.tril(B, -1).transpose(-1, -2)).contiguous()
    H = torch.complex(A, B).contiguous()
    N, name = shape[-1], "x".join(str(s) for s in shape)
    fmt = "median %.2f ms (min %.2f max %.2f, %d runs)"
    if not embedding:
        f = _time(lambda: dev.herm_tridiag_factor(H), h)
        print("%s: herm_tridiag_factor " % name + fmt % f, flush=True)
    rows = {}
    for sub in (None, (0, 8)):
        rows[sub] = (_time(lambda: dev.eigen_herm(H, subset=sub), h), _time(lambda: dev.eigenvals_herm(H, subset=sub), h))
        if not embedding:
            print("%s subset=%s: eigen_herm " % (name, sub) + fmt % rows[sub][0] + "  eigenvals_herm " + fmt % rows[sub][1], flush=True)
    if embedding:
        E = torch.cat([torch.cat([A, -B], -1), torch.cat([B, A], -1)], -2).contiguous()
        del A, B, H
        for red in ("tridiag", None):
            for sub, sube in ((None, None), ((0, 8), (0, 16))):          # every eigenvalue of the embedding comes twice
                full = _time(lambda: dev.eigen_sym(E, reduction=red, subset=sube), h)
                vals = _time(lambda: dev.eigenvals_sym(E, reduction=red, subset=sube), h)
                print("%s subset=%s: embedding of order %d, eigen_sym(reduction=%s) " % (name, sube, 2 * N, red) + fmt % full + "  eigenvals_sym "
                      + fmt % vals + "   eigen_herm / it: %.2f  eigenvals_herm / it: %.2f" % (rows[sub][0][0] / full[0], rows[sub][1][0] / vals[0]), flush=True)
        return
    if 2 * N > 2048:
        print("%s: the embedding of order %d is beyond the family's limit of 2048" % (name, 2 * N), flush=True)
    Hh = H.cpu().numpy()
    t0 = time.perf_counter()
    np.linalg.eigh(Hh)
    host = (time.perf_counter() - t0) * 1e3
    print("%s: numpy.linalg.eigh on the host %.1f ms (one run, wall clock)   eigen_herm / it: %.3f" % (name, host, rows[None][0][0] / host), flush=True)


if __name__ == "__main__":
    main()
