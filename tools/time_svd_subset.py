"""Time the selected-triplet SVD beside the full routes, each shape in a child process of its own: svd_decomp(A, subset=(0, 8)),
svd_vals(A, subset=(0, 8)) and svd_vals(A) against svd_decomp(A, algo='dc') and the default route (whose results would be sliced),
at 512^2, 1024^2, 2048^2, 64 x 512^2 and 1024 x 64^2, with the stage split of the subset call (nd4hip_dgesvdx_last_stages); then
bidiag_svd(d, e, subset=(0, 8)) against the full bidiag_svd at K = 2048 and at 1024 x 64; then, without a bound, the relative
error of every singular value of graded_40 (tests/svd_dc_common.py) against numpy.linalg.svd of the same bidiagonal, for the
bisection and for the full solver. HIP events, median of 10 after warm-ups (a call of more than half a second: median of 3).
usage: python tools/time_svd_subset.py            (every shape, one child each)
       python tools/time_svd_subset.py <shape>    (one of 512x512, ..., bidiag_2048, bidiag_1024x64, graded_40)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 512), (1024, 1024), (2048, 2048), (64, 512, 512), (1024, 64, 64)]
JOBS = ["x".join(str(s) for s in shape) for shape in SHAPES] + ["bidiag_2048", "bidiag_1024x64", "graded_40"]
FMT = "median %.2f ms (min %.2f max %.2f, %d runs)"


def _time(fn, h):
    """(median, min, max, reps): the first call decides how many more are affordable"""
    from bench_ops import _median_ms
    first = _median_ms(fn, h, reps=1, warm=1)[0]
    reps, warm = (10, 2) if first <= 500.0 else (3, 0)
    return _median_ms(fn, h, reps=reps, warm=warm) + (reps,)


def _stages(fn, h, reps):
    h.profile_enable(True)
    try:
        runs = []
        for _ in range(reps):
            fn()
            runs.append(h.svd_subset_last_stages())
    finally:
        h.profile_enable(False)
    med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}
    return "  ".join("%s %.2f" % kv for kv in med.items()) + "  sum %.2f" % sum(med.values())


def dense(name):
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    A = dev.fill_uniform(7, tuple(int(s) for s in name.split("x")))
    dc = _time(lambda: dev.svd_decomp(A, algo="dc"), h)
    jac = _time(lambda: dev.svd_decomp(A), h)
    print(("%s full: algo='dc' " + FMT + "  default route " + FMT) % ((name,) + dc + jac), flush=True)
    for what, fn in (("svd_decomp(A, subset=(0, 8))", lambda: dev.svd_decomp(A, subset=(0, 8))), ("svd_vals(A, subset=(0, 8))", lambda: dev.svd_vals(A, subset=(0, 8))),
                     ("svd_vals(A)", lambda: dev.svd_vals(A))):
        t = _time(fn, h)
        print(("%s %s: " + FMT + " = %.2f of algo='dc', %.2f of the default route") % ((name, what) + t + (t[0] / dc[0], t[0] / jac[0])), flush=True)
    print("  stages of svd_decomp(A, subset=(0, 8)) (ms, median of 5): " + _stages(lambda: dev.svd_decomp(A, subset=(0, 8)), h, 5), flush=True)
    print("  stages of svd_vals(A) (ms, median of 5): " + _stages(lambda: dev.svd_vals(A), h, 5), flush=True)


def bidiag(name):
    from nd4js_amd import _lib, dev
    h = _lib.handle(0)
    lead, K = ((), 2048) if name == "bidiag_2048" else ((1024,), 64)
    d, e = dev.fill_uniform(8, lead + (K,)), dev.fill_uniform(9, lead + (K,))
    full = _time(lambda: dev.bidiag_svd(d, e), h)
    print(("%s (J = K + 1) bidiag_svd(d, e): " + FMT) % ((name,) + full), flush=True)
    info = {}
    dev.bidiag_svd(d, e, subset=(0, 8), info=info)
    print("%s members sent to the full solver with subset=(0, 8): %d of %d" % (name, int(info["fallback"].sum()), info["fallback"].numel()), flush=True)
    for what, fn in (("bidiag_svd(d, e, subset=(0, 8))", lambda: dev.bidiag_svd(d, e, subset=(0, 8))), ("bidiag_svdvals(d, e, subset=(0, 8))", lambda: dev.bidiag_svdvals(d, e, subset=(0, 8))),
                     ("bidiag_svdvals(d, e)", lambda: dev.bidiag_svdvals(d, e))):
        t = _time(fn, h)
        print(("%s %s: " + FMT + " = %.2f of the full bidiag_svd") % ((name, what) + t + (t[0] / full[0],)), flush=True)
    print("  stages of bidiag_svd(d, e, subset=(0, 8)) (ms, median of 5): " + _stages(lambda: dev.bidiag_svd(d, e, subset=(0, 8)), h, 5), flush=True)


def graded():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from svd_dc_common import PATH_CASES, bidiag_dense
    from nd4js_amd import la
    d, e = PATH_CASES["graded_40"]
    ref = np.linalg.svd(bidiag_dense(d, e), compute_uv=False)
    bis, full = la.bidiag_svdvals(d, e), la.bidiag_svd(d, e)[1]
    print("graded_40: relative error of each singular value against numpy.linalg.svd (index: bisection / full solver)")
    for i in range(len(ref)):
        print("  %2d  sv %.3e  %.2e / %.2e" % (i, ref[i], abs(bis[i] - ref[i]) / ref[i], abs(full[i] - ref[i]) / ref[i]))
    print("graded_40 largest relative error: bisection %.3g, full solver %.3g" % (np.max(np.abs(bis - ref) / ref), np.max(np.abs(full - ref) / ref)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        for job in JOBS:                                       # one process per shape, one after the other
            subprocess.run([sys.executable, os.path.abspath(__file__), job], check=True, timeout=900)
    elif sys.argv[1] == "graded_40":
        graded()
    elif sys.argv[1].startswith("bidiag_"):
        bidiag(sys.argv[1])
    else:
        dense(sys.argv[1])
