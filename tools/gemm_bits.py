#!/usr/bin/env python3
"""One line per seeded product with the SHA-256 of C's bytes, over every path of nd4_gemm (the shape list in the docstring of
tests/test_gpu_gemm_paths.py, with 4096^3, 1000^3, (64, 4096, 4096) and a batch). Two builds of the library that accumulate in the
same order print identical output: run it in both trees (python tools/gemm_bits.py > bits.txt) and compare the files."""
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nd4js_amd import _lib, dev  # noqa: E402

NN, TN, NT, TT = (0, 0), (1, 0), (0, 1), (1, 1)
# (transposes, M, N, K, alpha, beta, ld padding, base shift of A in elements)
CASES = (
    [(NN, 65, 33, 17, -1.0, 1.0, 1, 1), (NT, 130, 100, 32, 1.0, 0.0, 1, 1), (NN, 130, 100, 33, -1.0, 1.0, 2, 0), (TN, 130, 100, 16, -1.0, 1.0, 2, 0)] +       # rank-k and its neighbours
    [(t, m, n, k, 0.75, -0.5, 2, 0) for t in (NN, TN, NT, TT) for m, n, k in ((128, 128, 48), (256, 384, 64), (384, 256, 160), (256, 256, 16), (128, 256, 32))] +  # tiled FULL
    [(NN, 1408, 1664, 48, 2.0, 1.0, 2, 0), (NN, 2176, 384, 48, -1.0, 0.0, 2, 0)] +                                                                      # tile map
    [(t, m, n, k, 2.0, 1.0, 2, 0) for t in (NN, TN, NT, TT) for m, n, k in ((130, 258, 34), (254, 126, 50), (2, 2, 34), (1410, 1666, 36))] +              # tiled edge
    [(t, m, n, k, -0.5, 2.0, 1, 1) for t in (NN, TN, NT, TT) for m, n, k in ((150, 94, 70), (129, 17, 255), (301, 97, 203))] +                            # tiled scalar
    [(t, m, n, k, 0.75, b, 2, 0) for t in (NN, TT) for b in (0.0, 0.5) for m, n, k in ((64, 200, 512), (16, 16, 8192), (16, 16, 9001), (130, 70, 2001))] +  # split-K
    [(t, m, n, k, 2.0, 0.5, 2, 0) for t in (NN, TN, NT, TT) for m, n, k in ((128, 128, 4096), (256, 256, 2048))] +
    [(NN, 1280, 2048, 512, 0.75, -0.5, 0, 0), (NN, 5, 7, 0, 0.75, 0.5, 2, 0)] +                                                                          # 160 tiles split; K = 0
    [(NN, 4096, 4096, 4096, 1.0, 0.0, 0, 0), (NN, 1000, 1000, 1000, 1.0, 0.0, 0, 0), (NN, 64, 4096, 4096, 1.0, 0.0, 0, 0)])


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def main():
    torch.cuda.set_device(0)
    h = _lib.handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    for n, ((ta, tb), M, N, K, alpha, beta, pad, shift) in enumerate(CASES):
        ar, ac = (K, M) if ta else (M, K)
        br, bc = (N, K) if tb else (K, N)
        lda, ldb, ldc = ac + pad, bc + pad, N + pad
        A = dev.fill_uniform(100 + 3 * n, (ar * lda + 2,))
        B = dev.fill_uniform(101 + 3 * n, (br * ldb + 2,))
        C = dev.fill_uniform(102 + 3 * n, (M, ldc))
        pA = ctypes.c_void_p(A.data_ptr() + 8 * shift)
        _lib.check(h.lib.nd4hip_dgemm_ex_dev(h.ptr, ta, tb, M, N, K, alpha, pA, lda, ctypes.c_void_p(B.data_ptr()), ldb, beta,
                                             ctypes.c_void_p(C.data_ptr()), ldc))
        print("ex %s%s %5d %5d %5d alpha %5.2f beta %5.2f ld+%d shift %d  %s" % ("NT"[ta], "NT"[tb], M, N, K, alpha, beta, pad, shift, sha(C)), flush=True)
    for batch, I, K, J in ((5, 70, 24, 50), (3, 50, 40, 30), (3, 100, 2000, 60), (4, 1280, 512, 1024), (6, 256, 208, 128)):
        A = dev.fill_uniform(900 + batch, (batch, I, K))
        B = dev.fill_uniform(901 + batch, (batch, K, J))
        print("matmul2 batch %d %5d %5d %5d  %s" % (batch, I, K, J, sha(dev.matmul2(A, B))), flush=True)


if __name__ == "__main__":
    main()
