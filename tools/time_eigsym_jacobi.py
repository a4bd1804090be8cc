"""Time both routes of eigen_sym / eigenvals_sym in one run: algo='jacobi' (csrc/syevj.hip) beside the default route (csrc/syev.hip),
with vectors and values only, HIP events, median of 10 after 3 warm-ups, at 65536 x 8^2, 4096 x 32^2, 1024 x 64^2, 256 x 128^2 and
one 64^2 matrix; the sweeps the Jacobi route needed are printed with each shape. With --accuracy the tables of DESIGN 4.18
follow: per graded positive definite case of tests/eigsym_jacobi_common.py the device's largest relative eigenvalue error, its
share of N eps kappa_2(A) and the default route's relative error on the same input; and the largest share of each bound of
tests/eigsym_common.py that the Jacobi route uses over its catalogue.
usage: python tools/time_eigsym_jacobi.py [--accuracy]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_ops import _median_ms

SHAPES = [(65536, 8, 8), (4096, 32, 32), (1024, 64, 64), (256, 128, 128), (64, 64)]


def timings():
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    for shape in SHAPES:
        A = dev.fill_uniform(7, shape)
        S = torch.tril(A) + torch.tril(A, -1).transpose(-1, -2)
        name = "x".join(str(s) for s in shape)
        info = {}
        dev.eigen_sym(S, algo="jacobi", info=info)
        sw = info["sweeps"].reshape(-1)
        jf = _median_ms(lambda: dev.eigen_sym(S, algo="jacobi"), h, reps=10, warm=3)
        jv = _median_ms(lambda: dev.eigenvals_sym(S, algo="jacobi"), h, reps=10, warm=3)
        df = _median_ms(lambda: dev.eigen_sym(S), h, reps=10, warm=3)
        dv = _median_ms(lambda: dev.eigenvals_sym(S), h, reps=10, warm=3)
        print("%s sweeps %d..%d" % (name, int(sw.min()), int(sw.max())), flush=True)
        for what, t in (("jacobi eigen_sym", jf), ("jacobi eigenvals_sym", jv), ("default eigen_sym", df), ("default eigenvals_sym", dv)):
            print("  %-22s median %.3f ms (min %.3f max %.3f)" % ((what,) + t), flush=True)
        print("  default / jacobi: eigen_sym %.2f  eigenvals_sym %.2f" % (df[0] / jf[0], dv[0] / jv[0]), flush=True)


def accuracy():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import eigsym_common as C
    import eigsym_jacobi_common as J
    from nd4js_amd import la
    for name in sorted(J.GRADED, key=lambda n: J.GRADED[n][0]):
        S = J.case(name)[0]
        N = S.shape[-1]
        ref = J.graded_reference(name)
        bound = N * J.EPS * J.scaled_kappa(S)
        err = (np.abs(la.eigenvals_sym(S, algo="jacobi") - ref) / ref).max()
        err_default = (np.abs(la.eigenvals_sym(S) - ref) / ref).max()
        print("%s N %d cond %.1e: jacobi relative error %.3g = %.3g of N eps kappa_2(A) = %.3g; default route %.3g"
              % (name, N, ref[0] / ref[-1], err, err / bound, bound, err_default), flush=True)
    worst = [0.0, 0.0, 0.0]
    for name in J.names():
        S = J.case(name)[0]
        lam, V = la.eigen_sym(S, algo="jacobi")
        worst = [max(a, b) for a, b in zip(worst, C.shares(S, lam, V, J.lapack(name)[0]))]
    print("largest shares of the bounds of eigsym_common over the catalogue (values, residual, orthogonality): %.3g %.3g %.3g" % tuple(worst), flush=True)


if __name__ == "__main__":
    timings()
    if "--accuracy" in sys.argv:
        accuracy()
