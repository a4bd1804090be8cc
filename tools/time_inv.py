"""Time inv, tril_inv and cholesky_inv beside what a user did before them, in one run: HIP events on device-resident arrays, median of 10
after 3 warm-ups (a call of more than half a second: median of 3).
  inv(A)           against lu_solve(*lu_decomp(A), I) and numpy.linalg.inv on the host (wall clock, one run);
  tril_inv(L)      against dev.tri_solve(L, I, upper=False), the device form of tril_solve(L, I);
  cholesky_inv(L)  against cholesky_solve(L, I).
The identities of the old routes are built once, outside the timed calls. Shapes: 65536 x 8^2, 1024 x 32^2, 1024 x 64^2, 256 x 128^2,
64 x 512^2, 512^2, 1024^2, 2048^2, each in a child process of its own. Every ratio is new / old; above 1 the new route loses.
usage: python tools/time_inv.py [largest N, default 2048]     all shapes up to that N
       python tools/time_inv.py --shape 64x512x512             one shape, in this process"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(65536, 8, 8), (1024, 32, 32), (1024, 64, 64), (256, 128, 128), (64, 512, 512), (512, 512), (1024, 1024), (2048, 2048)]


def _time(fn, h):
    """(median, min, max, reps): the first call decides how many more are affordable"""
    first = _median_ms(fn, h, reps=1, warm=1)[0]
    reps, warm = (10, 3) if first <= 500.0 else (3, 0)
    return _median_ms(fn, h, reps=reps, warm=warm) + (reps,)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        return one(tuple(int(x) for x in sys.argv[2].split("x")))
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    for shape in SHAPES:
        if shape[-1] <= top:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "x".join(str(x) for x in shape)], check=True)


def one(shape):
    import numpy as np
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    N, name = shape[-1], "x".join(str(s) for s in shape)
    eye = torch.eye(N, dtype=torch.float64, device="cuda")
    A = dev.fill_uniform(7, shape)
    # a well-conditioned lower factor: unit-scale diagonal, small strict part
    L = (torch.tril(dev.fill_uniform(8, shape), -1) / (4.0 * N ** 0.5) + eye * 1.5).contiguous()
    I = eye.expand(shape).contiguous()
    fmt = "median %.3f ms (min %.3f max %.3f, %d runs)"
    info = {}
    rows = (("inv", lambda: dev.inv(A, info=info), "lu_solve(*lu_decomp(A), I)", lambda: dev.lu_solve(*dev.lu_decomp(A), I)),
            ("tril_inv", lambda: dev.tril_inv(L), "tri_solve(L, I, upper=False)", lambda: dev.tri_solve(L, I, False)),
            ("cholesky_inv", lambda: dev.cholesky_inv(L), "cholesky_solve(L, I)", lambda: dev.cholesky_solve(L, I)))
    for new_name, new, old_name, old in rows:
        tn, to = _time(new, h), _time(old, h)
        print("%s: %s " % (name, new_name) + fmt % tn + "   %s " % old_name + fmt % to + "   new / old: %.2f" % (tn[0] / to[0]), flush=True)
        if len(shape) == 2:
            # the kernels of one call, from a kernel trace (torch.profiler): every kernel's share of the kernel time
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                new()
                torch.cuda.synchronize()
            us = lambda e: float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))   # noqa: E731
            ks = sorted(((e.key.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split(" ")[-1][:20], us(e), e.count) for e in prof.key_averages() if us(e) > 0.0),
                        key=lambda r: -r[1])
            total = sum(t for _, t, _ in ks)
            print("%s: kernels of one %s %.3f ms: %s" % (name, new_name, total * 1e-3, ", ".join("%s %.0f %% (%d)" % (k, 100.0 * t / total, c) for k, t, c in ks[:8])),
                  flush=True)
        if new_name == "inv":
            Ah = A.cpu().numpy()
            t0 = time.perf_counter()
            np.linalg.inv(Ah)
            host = (time.perf_counter() - t0) * 1e3
            print("%s: numpy.linalg.inv on the host %.1f ms (one run, wall clock)   inv / it: %.3f" % (name, host, tn[0] / host), flush=True)


if __name__ == "__main__":
    main()
