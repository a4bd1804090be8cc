"""Times of schur_eigen and eigen_balance_pre on the device (device-resident inputs, HIP events around the _dev entry points):
schur_eigen at 512^2 / 1024^2 / 2048^2 and 1024 x 64^2, eigen_balance_pre at 2048^2. The inputs are quasi-triangular T with a
2x2 block every 16 rows and a diagonal of distinct values, Q from the device's qr_decomp, and a graded matrix for the balancing.
Every case runs in a child process of its own under its own time limit, and a case that fails ends the run. Prints one JSON line
per case: median of `reps` runs after one warm-up.

    python tools/time_eigvec.py [reps]            # all cases
    python tools/time_eigvec.py --case I [reps]   # one case, in this process"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

CASES = [("schur_eigen", (512, 512), 60), ("schur_eigen", (1024, 1024), 90), ("schur_eigen", (2048, 2048), 240),
         ("schur_eigen", (1024, 64, 64), 60), ("eigen_balance_pre", (2048, 2048), 120)]


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def one(idx, reps):
    import torch
    from nd4js_amd import dev
    op, shape, _ = CASES[idx]
    N = shape[-1]
    A = dev.fill_uniform(11 + idx, shape)
    if op == "schur_eigen":
        T = torch.triu(A)
        k = torch.arange(N, device=A.device, dtype=torch.float64)
        T.diagonal(dim1=-2, dim2=-1).copy_(2.0 * ((k * 7919) % N) - N)            # distinct, at least 2 apart, in scrambled order
        i = torch.arange(0, N - 1, 16, device=A.device)
        T[..., i + 1, i + 1] = T[..., i, i]
        T[..., i, i + 1] = 0.75
        T[..., i + 1, i] = -0.5
        Q = dev.qr_decomp(dev.fill_uniform(5 + idx, shape))[0]
        fn = lambda: dev.schur_eigen(Q, T)
    else:
        g = torch.arange(N, device=A.device, dtype=torch.float64)
        A = A * torch.exp2(torch.clamp(3.0 * (g[:, None] - g[None, :]), -900, 900) / 8.0)
        fn = lambda: dev.eigen_balance_pre(A, 2)
    ms = timed(fn, reps if N < 2048 else min(reps, 3))
    print(json.dumps({"op": op, "shape": list(shape), "ms": round(ms, 4)}), flush=True)


def main(reps):
    for idx, (_, _, limit) in enumerate(CASES):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", str(idx), str(reps)])
        if r.returncode != 0:
            print(json.dumps({"op": CASES[idx][0], "shape": list(CASES[idx][1]), "failed": r.returncode}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        one(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 10)
    else:
        sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 10))
