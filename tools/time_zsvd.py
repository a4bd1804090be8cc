"""Time the complex SVD beside what a user had before it: HIP events on device-resident arrays, median of 10 after 3 warm-ups, each
shape in a child process of its own.
  zbidiag_factor(A) (the reduction; for 3 M >= 5 N the route reduces R instead), zsvd_vals(A) (reduction + bisection), zsvd_decomp(A)
  (reduction + divide & conquer + both back-transformations): solver = vals - reduction, back-transformation ~ decomp - vals;
  the real svd_decomp(algo='dc') at the same shape (a quarter of the flops: context, not a competitor);
  svd_decomp(algo='dc') on the real embedding [[Re, -Im], [Im, Re]] of order 2 M x 2 N (where 2 max(M, N) <= 2048);
  numpy.linalg.svd on the host: wall clock of the second run, on at most 64 members and scaled to the batch ("~": extrapolated).
Every ratio is the complex route / the other; above 1 the new route loses.
usage: python tools/time_zsvd.py [largest M, default 2048]"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 32, 32), (1024, 64, 64), (64, 256, 256), (256, 512, 64), (512, 512), (1024, 1024), (2048, 256), (2048, 2048)]
HOST_CAP = 64


def one(shape):
    import numpy as np
    import torch
    from bench_ops import _median_ms
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    ms = lambda fn: _median_ms(fn, h, reps=10, warm=3)[0]     # noqa: E731
    M, N = shape[-2:]
    rng = np.random.default_rng(1)
    A = torch.from_numpy(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).cuda()
    At = A if M >= N else A.conj().transpose(-1, -2).contiguous()
    red, vals, dec = ms(lambda: dev.zbidiag_factor(At)), ms(lambda: dev.zsvd_vals(A)), ms(lambda: dev.zsvd_decomp(A))
    Ar = A.real.contiguous()
    real = ms(lambda: dev.svd_decomp(Ar, algo="dc"))
    emb = float("nan")
    if 2 * max(M, N) <= 2048:
        E = torch.cat([torch.cat([A.real, -A.imag], -1), torch.cat([A.imag, A.real], -1)], -2).contiguous()
        emb = ms(lambda: dev.svd_decomp(E, algo="dc"))
    batch = A.numel() // (M * N)
    Ah = A.reshape((-1, M, N))[:HOST_CAP].cpu().numpy()
    np.linalg.svd(Ah, full_matrices=False)
    t0 = time.perf_counter()
    np.linalg.svd(Ah, full_matrices=False)
    host = (time.perf_counter() - t0) * 1e3 * batch / len(Ah)
    print("%-14s %9.3f %9.3f %9.3f | %9.3f %6.2f | %9.3f %6.2f | %s%.1f %6.3f" % ("x".join(map(str, shape)), red, vals, dec, real, dec / real, emb, dec / emb,
                                                                                 "~" if batch > len(Ah) else "", host, dec / host), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        return one(tuple(int(x) for x in sys.argv[2].split("x")))
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    print("%-14s %9s %9s %9s | %9s %6s | %9s %6s | %s" % ("shape", "reduction", "vals", "decomp", "real dc", "ratio", "embedding", "ratio", "numpy svd, ratio"),
          flush=True)
    for shape in SHAPES:
        if max(shape[-2:]) <= top:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "x".join(map(str, shape))], timeout=300).returncode
            if rc != 0:
                sys.exit("shape %s ended with status %d: nothing more is started" % (shape, rc))


if __name__ == "__main__":
    main()
