"""Time schur_sylvester and sylvester_solve per tier, in one run: HIP events on device-resident arrays, median of 10 after 3 warm-ups (a call
of more than half a second: median of 3). A = (U - 1/2) 2 / sqrt(N) + 2 I with U uniform, B likewise, so the spectra stay near 2; TA and
TB are their upper triangles with a 2x2 block (a subdiagonal entry -0.3) at every third row. Up to N = 512 also sylvester_solve(A, B, C),
the two schur_decomp calls that it contains, and the share of the triangular stage and of the decompositions in the whole solve (above,
one schur_decomp of one matrix takes 8 s and more on its one workgroup: not timed). For a single member also every kernel's share of the
kernel time of one schur_sylvester. Shapes: 4096 x 32^2, 1024 x 64^2, 256 x 128^2, 512^2, 1024^2, 2048^2, each in a child process of its own.
usage: python tools/time_sylvester.py [largest N, default 2048]     all shapes up to that N
       python tools/time_sylvester.py --shape 1024x64x64             one shape, in this process"""
import os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(4096, 32, 32), (1024, 64, 64), (256, 128, 128), (512, 512), (1024, 1024), (2048, 2048)]


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
    import torch
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    N, name = shape[-1], "x".join(str(s) for s in shape)
    eye = torch.eye(N, dtype=torch.float64, device="cuda")
    A, B = (((dev.fill_uniform(seed, shape) - 0.5) * (2.0 / N ** 0.5) + 2.0 * eye).contiguous() for seed in (7, 8))
    C = dev.fill_uniform(9, shape)
    sub = torch.diag_embed(torch.tensor([-0.3 if i % 3 == 0 else 0.0 for i in range(N - 1)], dtype=torch.float64, device="cuda"), offset=-1)
    TA, TB = (torch.triu(A) + sub).contiguous(), (torch.triu(B) + sub).contiguous()
    info = {}
    fmt = "median %.3f ms (min %.3f max %.3f, %d runs)"
    tri = _time(lambda: dev.schur_sylvester(TA, TB, C, info=info), h)
    trt = _time(lambda: dev.schur_sylvester(TA, TB, C, trans_b=True, info=info), h)
    print("%s: schur_sylvester " % name + fmt % tri + "   trans_b " + fmt % trt, flush=True)
    if N <= 512:
        whole = _time(lambda: dev.sylvester_solve(A, B, C, info=info), h)
        schur = _time(lambda: (dev.schur_decomp(A), dev.schur_decomp(B)), h)
        print("%s: sylvester_solve " % name + fmt % whole + "   two schur_decomp " + fmt % schur +
              "   shares of the solve: triangular stage %.3f, decompositions %.3f" % (tri[0] / whole[0], schur[0] / whole[0]), flush=True)
    if len(shape) == 2:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            dev.schur_sylvester(TA, TB, C, info=info)
            torch.cuda.synchronize()
        us = lambda e: float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))   # noqa: E731
        ks = sorted(((e.key.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1].split(" ")[-1][:20], us(e), e.count)
                     for e in prof.key_averages() if us(e) > 0.0), key=lambda r: -r[1])
        total = sum(t for _, t, _ in ks)
        print("%s: kernels of one schur_sylvester %.3f ms: %s" % (name, total * 1e-3, ", ".join("%s %.0f %% (%d)" % (k, 100.0 * t / total, c) for k, t, c in ks[:6])),
              flush=True)


if __name__ == "__main__":
    main()
