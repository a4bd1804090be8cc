"""Time the generalised Hermitian-definite eigenproblem beside its parts and beside what a user had before it, in one run: HIP events
on device-resident arrays, median of 10 after 3 warm-ups (a call of more than half a second: median of 3).
  herm_cholesky_decomp(B); eigen_herm_gen and eigenvals_herm_gen, full and with subset=(0, 8);
  eigen_herm alone on the same C = L^-1 A L^-H (what is left is the overhead of the factorisation, reduction and back-transformation);
  the composition of the public calls: herm_cholesky_decomp, two ztril_solve around a conjugate transposition, eigen_herm,
  ztril_solve(adjoint=True);
  the real embedding [[Re, -Im], [Im, Re]] of order 2 N of both matrices through eigen_sym_gen (where 2 N <= 2048);
  scipy.linalg.eigh(A, B) of the same matrices on the host (wall clock, one run).
Shapes: 65536 x 8^2, 1024 x 16^2, 1024 x 32^2, 1024 x 64^2 (the three candidates for the fused tier's edge), 64 x 512^2, 512^2, 1024^2,
2048^2, each in a child process of its own. Every line ends with the ratio eigen_herm_gen / the other; above 1 the new route loses.
usage: python tools/time_hegv.py [largest N, default 2048]     all shapes up to that N
       python tools/time_hegv.py --shape 64x512x512            one shape, in this process"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(65536, 8, 8), (1024, 16, 16), (1024, 32, 32), (1024, 64, 64), (64, 512, 512), (512, 512), (1024, 1024), (2048, 2048)]


def _time(fn, h):
    """(median, min, max, reps): the first call decides how many more are affordable"""
    first = _median_ms(fn, h, reps=1, warm=1)[0]
    reps, warm = (10, 3) if first <= 500.0 else (3, 0)
    return _median_ms(fn, h, reps=reps, warm=warm) + (reps,)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        return one(tuple(int(x) for x in sys.argv[2].split("x")), "--embedding" in sys.argv)
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    for shape in SHAPES:
        if shape[-1] <= top:
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", "x".join(str(x) for x in shape)]
            subprocess.run(cmd, check=True)
            # the embedding in a process of its own: its workspace is most of the device's memory at 64 x 1024^2
            if 2 * shape[-1] <= 2048 and subprocess.run(cmd + ["--embedding"]).returncode != 0:
                print("%s: the embedding of order %d did not finish (see above)" % (cmd[-1], 2 * shape[-1]), flush=True)


def one(shape, embedding=False):
    import numpy as np
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    N, name = shape[-1], "x".join(str(s) for s in shape)
    re, im = dev.fill_uniform(7, shape), dev.fill_uniform(8, shape)
    A = torch.complex((torch.tril(re) + torch.tril(re, -1).transpose(-1, -2)).contiguous(),
                      (torch.tril(im, -1) - torch.tril(im, -1).transpose(-1, -2)).contiguous()).contiguous()
    G = torch.complex(dev.fill_uniform(9, shape), dev.fill_uniform(10, shape))
    B = (G @ G.conj().transpose(-1, -2) / N + torch.eye(N, dtype=torch.complex128, device="cuda")).contiguous()   # a Gram matrix plus I
    del re, im, G
    fmt = "median %.2f ms (min %.2f max %.2f, %d runs)"
    gen = {sub: (_time(lambda: dev.eigen_herm_gen(A, B, subset=sub), h), _time(lambda: dev.eigenvals_herm_gen(A, B, subset=sub), h))
           for sub in (None, (0, 8))}
    if embedding:
        emb = lambda M: torch.cat([torch.cat([M.real, -M.imag], -1), torch.cat([M.imag, M.real], -1)], -2).contiguous()  # noqa: E731
        Ae, Be = emb(A), emb(B)
        del A, B
        for sub, sube in ((None, None), ((0, 8), (0, 16))):                 # every eigenvalue of the embedding comes twice
            full = _time(lambda: dev.eigen_sym_gen(Ae, Be, subset=sube), h)
            vals = _time(lambda: dev.eigenvals_sym_gen(Ae, Be, subset=sube), h)
            print("%s subset=%s: embedding of order %d, eigen_sym_gen " % (name, sube, 2 * N) + fmt % full + "  eigenvals_sym_gen " + fmt % vals
                  + "   eigen_herm_gen / it: %.2f  eigenvals_herm_gen / it: %.2f" % (gen[sub][0][0] / full[0], gen[sub][1][0] / vals[0]), flush=True)
        return
    print("%s: herm_cholesky_decomp " % name + fmt % _time(lambda: dev.herm_cholesky_decomp(B), h), flush=True)
    for sub in (None, (0, 8)):
        print("%s subset=%s: eigen_herm_gen " % (name, sub) + fmt % gen[sub][0] + "  eigenvals_herm_gen " + fmt % gen[sub][1], flush=True)
    L = dev.herm_cholesky_decomp(B)
    C = dev.herm_gen_reduce(A, L)
    alone = _time(lambda: dev.eigen_herm(C), h)
    share = 1.0 - alone[0] / gen[None][0][0]
    print("%s: eigen_herm alone on the same C " % name + fmt % alone + "   the factorisation, reduction and back-transformation are %.1f %% of "
          "eigen_herm_gen (%.2f ms)" % (100.0 * share, gen[None][0][0] - alone[0]), flush=True)

    def composition():
        Lc = dev.herm_cholesky_decomp(B)
        W = dev.ztril_solve(Lc, A)                                          # (A is Hermitian in full here)
        Cc = dev.ztril_solve(Lc, W.conj().transpose(-1, -2).contiguous())
        lam, Y = dev.eigen_herm(Cc)
        return lam, dev.ztril_solve(Lc, Y, adjoint=True)
    comp = _time(composition, h)
    print("%s: the composition of the public calls " % name + fmt % comp + "   eigen_herm_gen / it: %.2f" % (gen[None][0][0] / comp[0]), flush=True)
    if 2 * N > 2048:
        print("%s: the embedding of order %d is beyond eigen_sym_gen's limit of 2048" % (name, 2 * N), flush=True)
    try:
        import scipy.linalg
    except ImportError:
        return print("%s: scipy is not installed: no host column" % name, flush=True)
    Ah, Bh = A.cpu().numpy().reshape(-1, N, N), B.cpu().numpy().reshape(-1, N, N)
    t0 = time.perf_counter()
    for a, b in zip(Ah, Bh):
        scipy.linalg.eigh(a, b)
    host = (time.perf_counter() - t0) * 1e3
    print("%s: scipy.linalg.eigh(A, B) on the host %.1f ms (one run, wall clock)   eigen_herm_gen / it: %.3f" % (name, host, gen[None][0][0] / host), flush=True)


if __name__ == "__main__":
    main()
