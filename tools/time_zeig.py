"""Time the general complex eigenproblem beside what a user had before it: HIP events on device-resident arrays, median of 10 after 3
warm-ups (of 3 after 1 at N = 512 and a single run after 1 at N = 1024, where a call takes seconds), each shape in a child process of
its own with a time limit sized to it; every figure is printed as soon as it is measured.
  zhess_decomp(A), zschur_decomp(A), zeigen(A), zeigenvals(A);
  the stages of zeigen on their own: zhess_decomp (reduction and Q), zschur_qr (iteration), zschur_eigen (back-substitution, Q X and the
  normalisation), as shares of their sum (each public stage carries its own copies and flag read-back: not the shares inside one call);
  at 64 x 256^2 and 512^2 the iteration (zschur_qr) with ND4HIP_ZHSEQR_EAGER=0, the per-sweep deferral, against ND4HIP_ZHSEQR_EAGER=1, every
  rotation applied everywhere as it is produced (the default when H is in global memory): deferred / eager, above 1 the deferral loses;
  the real eigen at the same shape (a quarter of the flops: context, not a competitor);
  numpy.linalg.eig on the host, what a user does today: wall clock of the second run, on at most 16 members and scaled to the batch
  ("~": extrapolated).
Every other ratio is the complex route / the other; above 1 the new route loses.
usage: python tools/time_zeig.py [largest N, default 1024]"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(65536, 8, 8), (1024, 32, 32), (1024, 64, 64), (64, 256, 256), (256, 256), (512, 512), (1024, 1024)]
AB_SHAPES = [(64, 256, 256), (512, 512)]
HOST_CAP = 16


def one(shape):
    import numpy as np
    import torch
    from bench_ops import _median_ms
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    N = shape[-1]
    reps, warm = (1, 1) if N >= 1024 else (3, 1) if N >= 512 else (10, 3)

    def ms(name, fn):
        v = _median_ms(fn, h, reps=reps, warm=warm)[0]
        print("  %s %s: %.3f ms" % ("x".join(map(str, shape)), name, v), flush=True)
        return v
    rng = np.random.default_rng(1)
    A = torch.from_numpy(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).cuda()
    hess, schur = ms("zhess_decomp", lambda: dev.zhess_decomp(A)), ms("zschur_decomp", lambda: dev.zschur_decomp(A))
    eig, vals = ms("zeigen", lambda: dev.zeigen(A)), ms("zeigenvals", lambda: dev.zeigenvals(A))
    Qh, Hs = dev.zhess_decomp(A)
    Q, T = dev.zschur_qr(Qh, Hs)
    it, back = ms("zschur_qr", lambda: dev.zschur_qr(Qh, Hs)), ms("zschur_eigen", lambda: dev.zschur_eigen(Q, T))
    ab = ""
    if tuple(shape) in AB_SHAPES:
        os.environ["ND4HIP_ZHSEQR_EAGER"] = "0"
        deferred = ms("zschur_qr, per-sweep deferral", lambda: dev.zschur_qr(Qh, Hs))
        os.environ["ND4HIP_ZHSEQR_EAGER"] = "1"
        eager = ms("zschur_qr, every rotation everywhere", lambda: dev.zschur_qr(Qh, Hs))
        del os.environ["ND4HIP_ZHSEQR_EAGER"]
        ab = " | deferred / eager %.3f / %.3f = %.2f" % (deferred, eager, deferred / eager)
    parts = hess + it + back
    Ar = A.real.contiguous()
    real = ms("real eigen", lambda: dev.eigen(Ar))
    batch = A.numel() // (N * N)
    Ah = A.reshape((-1, N, N))[:HOST_CAP].cpu().numpy()
    np.linalg.eig(Ah)
    t0 = time.perf_counter()
    np.linalg.eig(Ah)
    host = (time.perf_counter() - t0) * 1e3 * batch / len(Ah)
    print("%-14s %9.3f %9.3f %9.3f %9.3f | %4.2f %4.2f %4.2f | %9.3f %6.2f | %s%.1f %6.3f%s" % (
        "x".join(map(str, shape)), hess, schur, eig, vals, hess / parts, it / parts, back / parts, real, eig / real, "~" if batch > len(Ah) else "", host,
        eig / host, ab), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        return one(tuple(int(x) for x in sys.argv[2].split("x")))
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    print("%-14s %9s %9s %9s %9s | %14s | %9s %6s | %s" % ("shape", "zhess", "zschur", "zeigen", "zeigvals", "red / it / vec", "real eigen", "ratio",
                                                         "numpy eig, ratio"), flush=True)
    for shape in SHAPES:
        if shape[-1] <= top:
            limit = 1100 if shape[-1] >= 1024 else 400        # 1024^2: about 30 calls of up to 15 s
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "x".join(map(str, shape))], timeout=limit).returncode
            except subprocess.TimeoutExpired:
                sys.exit("shape %s ran past its limit of %d s: nothing more is started" % (shape, limit))
            if rc != 0:
                sys.exit("shape %s ended with status %d: nothing more is started" % (shape, rc))


if __name__ == "__main__":
    main()
