"""Time the complex QR beside what a user had before it, in one run: HIP events on device-resident arrays, median of 10 after 3 warm-ups.
  zqr_factor(A), zqr_decomp(A), zqr_lstsq(A, Y) with K = 1 and with K = N;
  the real qr_decomp at the same M x N (a quarter of the flops: context, not a competitor);
  lstsq on the real embedding [[Re, -Im], [Im, Re]] of order 2 M x 2 N (where 2 M <= 2048);
  numpy.linalg.qr (batched) and numpy.linalg.lstsq (K = 1, member by member) on the host: wall clock of the second run, on at most
  256 members and scaled to the batch ("~": extrapolated).
One-matrix rows also give, from a kernel trace of one zqr_factor (torch.profiler), the split panel / zqr_vhc / zlu_update / rest and
zqr_vhc's rate against the fp64 matrix-core peak. The last line compares zqr_vhc with the route it replaces at one block of 2048 rows
against 2032 columns: V^H written out as a second array and the complex GEMM without transposition (kernel times of both).
Every ratio is the complex route / the other; above 1 the new route loses.
usage: python tools/time_zqr.py [largest M, default 2048]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import _median_ms

SHAPES = [(65536, 8, 8), (1024, 32, 32), (1024, 64, 64), (1024, 256, 32), (64, 512, 512), (512, 512), (1024, 1024), (2048, 2048), (2048, 256)]
PEAK_TFLOPS, NB, HOST_CAP = 78.6, 16, 256


def kernels(fn):
    """[(kernel name, microseconds)] of every kernel that fn launches, in launch order"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type.name == "CUDA" and (e.device_time_total or 0) > 0]
    return [(e.name, float(e.device_time_total)) for e in sorted(ev, key=lambda e: e.time_range.start)]


def main():
    import numpy as np
    import torch
    from nd4js_amd import _lib, dev
    top = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    h = _lib.handle(0)
    ms = lambda fn: _median_ms(fn, h, reps=10, warm=3)[0]     # noqa: E731
    print("%-16s %9s %9s %9s %9s | %9s %6s | %9s %6s | %10s %10s" % ("shape", "factor", "decomp", "lstsq K=1", "lstsq K=N", "qr_decomp", "ratio", "embedding",
                                                                      "ratio", "numpy qr", "np lstsq"))
    for shape in SHAPES:
        M, N = shape[-2:]
        if M > top:
            continue
        rng = np.random.default_rng(1)
        A = torch.from_numpy(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).cuda()
        Y1, YN = A[..., :1].contiguous(), A.clone()
        t = [ms(lambda: dev.zqr_factor(A)), ms(lambda: dev.zqr_decomp(A)), ms(lambda: dev.zqr_lstsq(A, Y1)), ms(lambda: dev.zqr_lstsq(A, YN))]
        Ar = A.real.contiguous()
        real = ms(lambda: dev.qr_decomp(Ar))
        emb = float("nan")
        if 2 * M <= 2048:
            E = torch.cat([torch.cat([A.real, -A.imag], -1), torch.cat([A.imag, A.real], -1)], -2).contiguous()
            Ye = torch.cat([Y1.real, Y1.imag], -2).contiguous()
            emb = ms(lambda: dev.lstsq(E, Ye))
        batch = A.numel() // (M * N)
        Ah, Yh = A.reshape((-1, M, N))[:HOST_CAP].cpu().numpy(), Y1.reshape((-1, M, 1))[:HOST_CAP].cpu().numpy()
        host = []
        for fn in (lambda: np.linalg.qr(Ah), lambda: [np.linalg.lstsq(a, y, rcond=None) for a, y in zip(Ah, Yh)]):
            fn()
            t0 = time.perf_counter()
            fn()
            host.append(("~" if batch > len(Ah) else "") + "%.1f" % ((time.perf_counter() - t0) * 1e3 * batch / len(Ah)))
        print("%-16s %9.3f %9.3f %9.3f %9.3f | %9.3f %6.2f | %9.3f %6.2f | %10s %10s" % ("x".join(map(str, shape)), t[0], t[1], t[2], t[3], real, t[1] / real, emb,
                                                                                        t[2] / emb, host[0], host[1]), flush=True)
        if batch == 1:
            rows = kernels(lambda: dev.zqr_factor(A))
            tot = sum(u for _, u in rows)
            part = {k: sum(u for n, u in rows if k in n) for k in ("zqr_panel", "zqr_vhc", "zlu_update")}
            flops = sum(8.0 * NB * (M - j0) * (N - j0 - NB + NB) for j0 in range(0, N - NB, NB))     # per block: V^H C and G = V^H V
            print("    kernels of one zqr_factor %.3f ms: panel %.3f, zqr_vhc %.3f, zlu_update %.3f, rest %.3f; zqr_vhc %.2f TFLOP/s = %.1f %% of the %.1f peak"
                  % (tot * 1e-3, part["zqr_panel"] * 1e-3, part["zqr_vhc"] * 1e-3, part["zlu_update"] * 1e-3, (tot - sum(part.values())) * 1e-3,
                     flops / part["zqr_vhc"] * 1e-6, 100.0 * flops / part["zqr_vhc"] * 1e-6 / PEAK_TFLOPS, PEAK_TFLOPS), flush=True)
    if top >= 2048:
        rng = np.random.default_rng(2)
        A = torch.from_numpy(rng.standard_normal((2048, NB)) + 1j * rng.standard_normal((2048, NB))).cuda()
        C = torch.from_numpy(rng.standard_normal((2048, 2032)) + 1j * rng.standard_normal((2048, 2032))).cuda()
        F, tau = dev.zqr_factor(A)
        dev.zqr_apply_q(F, tau, C, adjoint=True)
        vhc = max(u for n, u in kernels(lambda: dev.zqr_apply_q(F, tau, C, adjoint=True)) if "zqr_vhc" in n)     # the launch on C (the other: G)
        V = torch.tril(F, -1) + torch.eye(2048, NB, dtype=F.dtype, device=F.device)

        def stored():
            return dev.matmul2(V.conj().transpose(-1, -2).contiguous(), C)
        stored()
        old = kernels(stored)
        print("one block, 2048 rows x 2032 columns: zqr_vhc %.1f us (its partials are added by zqr_tw); V^H stored + complex GEMM %.1f us (%s); ratio %.2f"
              % (vhc, sum(u for _, u in old), ", ".join("%s %.1f" % (n.split("(")[0].split("::")[-1][:28], u) for n, u in old), vhc / sum(u for _, u in old)), flush=True)


if __name__ == "__main__":
    main()
