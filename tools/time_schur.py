"""Times of schur_decomp on the device, next to which README.md and DESIGN.md §4.12 put the reference's single-thread times:
batches 1024 x 64^2 and 64 x 256^2, and one matrix at 64, 128, 256, 512 and 1024 (one workgroup: correct, not fast). Inputs are
uniform(-1, 1) from the repo's generator. Per case: `ms` with device-resident inputs (HIP events around dev.schur_decomp, the
median of `reps` runs after a warm-up; one run for N >= 512) and, for one matrix, `host_ms`: the wall time of la.schur_decomp on a
numpy array, copies included, which is what install() weighs against the host module. eigen is timed on the 1024 x 64^2 batch.
Every case runs in a child process of its own under its own time limit, and a case that fails ends the run. One JSON line per case.

    python tools/time_schur.py [reps]            # all cases
    python tools/time_schur.py --case I [reps]   # one case, in this process"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

CASES = [("schur_decomp", (1024, 64, 64), 60), ("eigen", (1024, 64, 64), 60), ("schur_decomp", (64, 256, 256), 120),
         ("schur_decomp", (64, 64), 60), ("schur_decomp", (128, 128), 60), ("schur_decomp", (256, 256), 60),
         ("schur_decomp", (512, 512), 120), ("schur_decomp", (1024, 1024), 400)]


def timed(fn, reps):
    import torch
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
    from nd4js_amd import dev, la
    op, shape, _ = CASES[idx]
    N = shape[-1]
    A = dev.fill_uniform(31 + idx, shape)
    fn = (lambda: dev.eigen(A)) if op == "eigen" else (lambda: dev.schur_decomp(A))
    if N >= 512:
        dev.schur_decomp(dev.fill_uniform(3, (8, 8)))                             # the warm-up loads the code object only
        reps = 1
    else:
        fn()
    torch.cuda.synchronize()
    out = {"op": op, "shape": list(shape), "ms": round(timed(fn, reps), 4)}
    if len(shape) == 2 and N <= 512:
        Ah = A.cpu().numpy()
        t0 = time.perf_counter()
        _, _, sweeps = la.schur_decomp(Ah, sweeps=True)
        out["host_ms"] = round(1e3 * (time.perf_counter() - t0), 4)
        out["sweeps"] = sweeps
    print(json.dumps(out), flush=True)


def main(reps):
    for idx, (_, _, limit) in enumerate(CASES):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", str(idx), str(reps)])
        if r.returncode != 0:
            print(json.dumps({"op": CASES[idx][0], "shape": list(CASES[idx][1]), "failed": r.returncode}), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        one(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
