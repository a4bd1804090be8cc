"""Time the general complex LU and its solves beside what a user had before them, in one run: HIP events on device-resident arrays,
median of 10 after 3 warm-ups (a call of more than half a second: median of 3).
  zlu_decomp(A); zsolve(A, Y) with K = 1 and with K = N right-hand sides;
  the real embedding [[Re, -Im], [Im, Re]] of order 2 N through lu_decomp + lu_solve (where 2 N <= 4096, lu_decomp's limit);
  lu_decomp at the same N (a quarter of the flops of the complex factorisation: context, not a competitor);
  numpy.linalg.solve on the host (wall clock, one run).
One-matrix rows also give, from a kernel trace of one zlu_decomp (torch.profiler), the share of the trailing-update kernel in the kernel
time and its rate against the fp64 matrix-core peak.
Shapes: 65536 x 8^2, 1024 x 16^2 and 17^2 (the last order of the register tier and the first of the LDS tier), 1024 x 32^2, 1024 x 64^2, 64 x 512^2, 512^2, 1024^2, 2048^2, each in a child process of its own. Every ratio is
zsolve or zlu_decomp / the other; above 1 the new route loses.
usage: python tools/time_zlu.py [largest N, default 2048]     all shapes up to that N
       python tools/time_zlu.py --shape 64x512x512             one shape, in this process"""
import os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(65536, 8, 8), (1024, 16, 16), (1024, 17, 17), (1024, 32, 32), (1024, 64, 64), (64, 512, 512), (512, 512), (1024, 1024), (2048, 2048)]
PEAK_TFLOPS = 78.6                # fp64 matrix-core peak of one MI355X


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
    batch = int(np.prod(shape[:-2], dtype=np.int64))
    A = torch.complex(dev.fill_uniform(7, shape), dev.fill_uniform(8, shape)).contiguous()
    Y1 = torch.complex(dev.fill_uniform(9, shape[:-1] + (1,)), dev.fill_uniform(10, shape[:-1] + (1,))).contiguous()
    YN = torch.complex(dev.fill_uniform(11, shape), dev.fill_uniform(12, shape)).contiguous()
    fmt = "median %.3f ms (min %.3f max %.3f, %d runs)"
    dec = _time(lambda: dev.zlu_decomp(A), h)
    s1 = _time(lambda: dev.zsolve(A, Y1), h)
    sN = _time(lambda: dev.zsolve(A, YN), h)
    flops = batch * 8.0 / 3.0 * N ** 3
    print("%s: zlu_decomp " % name + fmt % dec + "  %.2f TFLOP/s" % (flops / dec[0] * 1e-9), flush=True)
    print("%s: zsolve K=1 " % name + fmt % s1 + "  zsolve K=N " % () + fmt % sN, flush=True)
    if batch == 1:
        # the trailing-update kernel alone, from a kernel trace of one zlu_decomp: its share of the kernel time and its rate
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            dev.zlu_decomp(A)
            torch.cuda.synchronize()
        us = lambda e: float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))   # noqa: E731
        rows = [(e.key, us(e)) for e in prof.key_averages() if us(e) > 0.0]
        total, upd = sum(t for _, t in rows), sum(t for k, t in rows if "zlu_update" in k)
        OB = N // (1 + sum(e.count for e in prof.key_averages() if "zlu_update" in e.key))   # one update per outer block but the last
        uflops = sum(8.0 * (N - j1) ** 2 * min(OB, N - j0) for j0 in range(0, N, OB) for j1 in [min(j0 + OB, N)])
        print("%s: kernels of one zlu_decomp %.3f ms; zlu_update %.3f ms = %.1f %% of them, %.2f TFLOP/s = %.1f %% of the %.1f peak; the rest: %s"
              % (name, total * 1e-3, upd * 1e-3, 100.0 * upd / total, uflops / upd * 1e-6, 100.0 * uflops / upd * 1e-6 / PEAK_TFLOPS, PEAK_TFLOPS,
                 ", ".join("%s %.3f" % (k.split("(")[0].split("::")[-1].split(" ")[-1][:24], t * 1e-3) for k, t in sorted(rows, key=lambda r: -r[1]) if "zlu_update" not in k)),
              flush=True)
    Ar = A.real.contiguous()
    ludec = _time(lambda: dev.lu_decomp(Ar), h)
    print("%s: lu_decomp (real, same N) " % name + fmt % ludec + "   zlu_decomp / it: %.2f" % (dec[0] / ludec[0]), flush=True)
    if 2 * N <= 4096:
        emb = lambda M: torch.cat([torch.cat([M.real, -M.imag], -1), torch.cat([M.imag, M.real], -1)], -2).contiguous()  # noqa: E731
        Ae = emb(A)
        for K, Y, z in ((1, Y1, s1), (N, YN, sN)):
            Ye = torch.cat([Y.real, Y.imag], -2).contiguous()

            def embedding():
                LUe, Pe = dev.lu_decomp(Ae)
                return dev.lu_solve(LUe, Pe, Ye)
            e = _time(embedding, h)
            print("%s K=%d: embedding of order %d, lu_decomp + lu_solve " % (name, K, 2 * N) + fmt % e + "   zsolve / it: %.2f" % (z[0] / e[0]), flush=True)
        del Ae
    else:
        print("%s: the embedding of order %d is beyond lu_decomp's limit of 4096" % (name, 2 * N), flush=True)
    Ah, Yh = A.cpu().numpy(), YN.cpu().numpy()
    t0 = time.perf_counter()
    np.linalg.solve(Ah, Yh)
    host = (time.perf_counter() - t0) * 1e3
    print("%s: numpy.linalg.solve(A, Y) K=N on the host %.1f ms (one run, wall clock)   zsolve / it: %.3f" % (name, host, sN[0] / host), flush=True)


if __name__ == "__main__":
    main()
