"""Time eigen_sym_gen / eigenvals_sym_gen (csrc/sygv.hip) on device-resident arrays, and beside each, in the same run: eigen_sym alone
on the same C = L^-1 A L^-T (what the solver costs without the generalised part), and the user-level composition of the same route
through dev (cholesky_decomp, two tri_solve around a transpose, eigen_sym, transpose and tri_solve), which is what a user had to
write before. HIP events, median of 10 after 3 warm-ups, at 65536 x 8^2 and 1024 x 64^2 (both algos), 64 x 512^2 and one 2048^2.
The last line per shape is the overhead of the generalised problem over eigen_sym alone and the composition's time over the fused
call's. The composition's results are compared with the fused call's before anything is timed.
usage: python tools/time_sygv.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_ops import _median_ms

SHAPES = [((65536, 8, 8), (None, "jacobi")), ((1024, 64, 64), (None, "jacobi")), ((64, 512, 512), (None,)), ((2048, 2048), (None,))]


def composition(dev, A, B, algo, vectors=True):
    L = dev.cholesky_decomp(B)
    W = dev.tri_solve(L, A, False)
    C = dev.tri_solve(L, dev.transpose(W), False)
    if not vectors:
        return dev.eigenvals_sym(C, algo=algo)
    lam, Y = dev.eigen_sym(C, algo=algo)
    return lam, dev.tri_solve(dev.transpose(L), Y, True)


def main():
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    for shape, algos in SHAPES:
        N = shape[-1]
        G = dev.fill_uniform(11, shape)
        A = torch.tril(G) + torch.tril(G, -1).transpose(-1, -2)
        X = dev.fill_uniform(12, shape)
        B = dev.matmul2(X, dev.transpose(X)) / N + torch.eye(N, dtype=torch.float64, device=A.device)
        B = (torch.tril(B) + torch.tril(B, -1).transpose(-1, -2)).contiguous()
        A = A.contiguous()
        C = dev._sygst(A, dev.cholesky_decomp(B))
        name = "x".join(str(s) for s in shape)
        for algo in algos:
            lam, Xf = dev.eigen_sym_gen(A, B, algo=algo)
            lc, Xc = composition(dev, A, B, algo)
            scale = float(lam.abs().max())
            print("%s algo=%s: fused vs composition max|dlambda| / max|lambda| = %.2e" % (name, algo or "dc", float((lam - lc).abs().max()) / scale), flush=True)
            rows = [("eigen_sym_gen", lambda: dev.eigen_sym_gen(A, B, algo=algo)),
                    ("eigen_sym alone on C", lambda: dev.eigen_sym(C, algo=algo)),
                    ("composition through dev", lambda: composition(dev, A, B, algo)),
                    ("eigenvals_sym_gen", lambda: dev.eigenvals_sym_gen(A, B, algo=algo)),
                    ("eigenvals_sym alone on C", lambda: dev.eigenvals_sym(C, algo=algo)),
                    ("composition, values only", lambda: composition(dev, A, B, algo, False))]
            t = {}
            for what, fn in rows:
                t[what] = _median_ms(fn, h, reps=10, warm=3)
                print("  %-26s median %.3f ms (min %.3f max %.3f)" % ((what,) + t[what]), flush=True)
            print("  with vectors: overhead over eigen_sym alone %.3f ms (x%.2f); composition / fused %.2f" % (
                t["eigen_sym_gen"][0] - t["eigen_sym alone on C"][0], t["eigen_sym_gen"][0] / t["eigen_sym alone on C"][0],
                t["composition through dev"][0] / t["eigen_sym_gen"][0]), flush=True)
            print("  values only:  overhead over eigenvals_sym alone %.3f ms (x%.2f); composition / fused %.2f" % (
                t["eigenvals_sym_gen"][0] - t["eigenvals_sym alone on C"][0], t["eigenvals_sym_gen"][0] / t["eigenvals_sym alone on C"][0],
                t["composition, values only"][0] / t["eigenvals_sym_gen"][0]), flush=True)


if __name__ == "__main__":
    main()
