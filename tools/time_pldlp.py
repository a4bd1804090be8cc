"""Times pldlp_decomp on each tier and pldlp_solve, next to ldl_decomp and solve at the same sizes, on device-resident arrays:

    python tools/time_pldlp.py [--quick] [--node <reference dist/nd.js> [--node-only]]

Shapes: 1024 x 64^2 and 64 x 512^2 (batches), one 512^2 / 1024^2 / 2048^2; pldlp_solve 2048^2 with 2048 right-hand sides. Each
line is one JSON record: the median of the repetitions of a host clock around calls that end in a device synchronise (the
factorisation reads its flags back, so it synchronises itself), after one warm-up call per shape and tier. A tier that cannot hold
the size, or whose run would take minutes (one workgroup on a 2048^2 matrix), is reported as skipped, never substituted. --node
times the reference's own pldlp_decomp at 512^2 and 1024^2 in a node process (one CPU thread), first; --node-only stops after it (no device needed). --quick halves the sizes' count for
a short GPU visit. The matrices are symmetric indefinite (the seeded generator, mirrored), so about a third of the steps are 2x2."""
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
QUICK = "--quick" in sys.argv
NODE_REF = sys.argv[sys.argv.index("--node") + 1] if "--node" in sys.argv else None


if NODE_REF:
    js = ("const nd=require(process.argv[1]);for(const n of [512,1024]){const a=new Float64Array(n*n);let s=12345;"
          "for(let i=0;i<n;i++)for(let j=0;j<=i;j++){s=(Math.imul(s,1103515245)+12345)>>>0;a[n*i+j]=a[n*j+i]=s/2147483648-1;}"
          "const S=new nd.NDArray(Int32Array.of(n,n),a);nd.la.pldlp_decomp(S);const t=process.hrtime.bigint();nd.la.pldlp_decomp(S);"
          "console.log(JSON.stringify({op:'pldlp_decomp',where:'reference, node, one CPU thread',batch:1,n,ms:Number(process.hrtime.bigint()-t)/1e6}));}")
    print(subprocess.run(["node", "-e", js, NODE_REF], stdout=subprocess.PIPE, text=True, check=True).stdout, end="", flush=True)
    if "--node-only" in sys.argv:
        sys.exit(0)


import torch  # noqa: E402

from nd4js_amd import dev, la  # noqa: E402

LIM = la.pldlp_limits()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def symmetric(seed, batch, n):
    G = dev.fill_uniform(seed, (batch, n, n))
    S = torch.tril(G) + torch.tril(G, -1).transpose(-1, -2)
    return S.contiguous()


def holds(tier, batch, n):
    if tier == "lds":
        return n <= LIM["lds_max_n"]
    if tier == "global":
        return n <= LIM["global_max_n"] and not (batch == 1 and n > 1024)      # one workgroup on 2048^2: minutes
    return batch * n <= 8192                                                    # grid: a batch loops over its members


shapes = [(1024, 64), (64, 512), (1, 512), (1, 1024)] + ([] if QUICK else [(1, 2048)])
for batch, n in shapes:
    S = symmetric(31 + n, batch, n)
    reps = 5 if batch * n * n * n < 2 ** 34 else 3
    auto = la.pldlp_tier(batch, n)
    for tier in ("lds", "global", "grid"):
        if not holds(tier, batch, n):
            emit(op="pldlp_decomp", batch=batch, n=n, tier=tier, skipped=True, auto=auto == tier)
            continue
        med, lo, hi = timed(lambda: dev.pldlp_decomp(S, tier=tier), reps)
        emit(op="pldlp_decomp", batch=batch, n=n, tier=tier, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), reps=reps, auto=auto == tier)
    # the parent's routes at the same size: ldl_decomp (no pivoting; made safe by a dominant diagonal) and solve (column-pivoted QR)
    Sd = S.clone()
    Sd.diagonal(dim1=-2, dim2=-1).add_(float(n))
    med, lo, hi = timed(lambda: dev.ldl_decomp(Sd), reps)
    emit(op="ldl_decomp", batch=batch, n=n, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), reps=reps)
    Y = dev.fill_uniform(5, (batch, n, 1))

    def qr_solve():                                   # what nd.la.solve does: rrqr_decomp, then rrqr_lstsq
        Q, R, Pq = dev.rrqr_decomp(S)
        return dev.rrqr_lstsq(Q, R, Pq, Y)
    med, lo, hi = timed(qr_solve, reps)
    emit(op="solve", batch=batch, n=n, rhs=1, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), reps=reps)
    med, lo, hi = timed(lambda: dev.pldlp_solve(*dev.pldlp_decomp(S), Y), reps)
    emit(op="pldlp_decomp+solve", batch=batch, n=n, rhs=1, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), reps=reps)
    LD, P = dev.pldlp_decomp(S)
    med, lo, hi = timed(lambda: dev.pldlp_solve(LD, P, Y), reps)
    emit(op="pldlp_solve", batch=batch, n=n, rhs=1, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), reps=reps)

n = 1024 if QUICK else 2048
S = symmetric(77, 1, n)[0]
LD, P = dev.pldlp_decomp(S)
Y = dev.fill_uniform(9, (n, n))
med, lo, hi = timed(lambda: dev.pldlp_solve(LD, P, Y), 3)
emit(op="pldlp_solve", batch=1, n=n, rhs=n, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), reps=3)
X = dev.pldlp_solve(LD, P, Y)
R = dev.matmul2(S, X) - Y
emit(op="pldlp_solve_check", n=n, backward_error=float(R.norm() / (S.norm() * X.norm() + Y.norm())))
