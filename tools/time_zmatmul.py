"""Times of the complex matmul2 pairings on the device (device-resident inputs, HIP events around dev.matmul2):
CC, CR and RC at 4096^2, a batch of 1024 x 128^2 CC and the skinny CC (64 x 4096) (4096 x 64). Prints one JSON line per case:
median of `reps` runs after one warm-up, with TFLOP/s counted as the reference's real flops (8 IKJ for CC, 4 IKJ for CR / RC)
and the fraction of the nominal fp64 MFMA peak (78.6 TFLOP/s)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nd4js_amd import dev  # noqa: E402

PEAK = 78.6e12


def timed(fn, reps):
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


def operand(seed, shape, cplx):
    if not cplx:
        return dev.fill_uniform(seed, shape)
    return torch.view_as_complex(dev.fill_uniform(seed, tuple(shape) + (2,)))


def main(reps=10):
    out = []
    cases = [("CC", (4096, 4096), (4096, 4096)), ("CR", (4096, 4096), (4096, 4096)), ("RC", (4096, 4096), (4096, 4096)),
             ("CC", (1024, 128, 128), (1024, 128, 128)), ("CC", (64, 4096), (4096, 64))]
    for pairing, sa, sb in cases:
        A = operand(1, sa, pairing[0] == "C")
        B = operand(2, sb, pairing[1] == "C")
        C = dev.matmul2(A, B)
        ms = timed(lambda: dev.matmul2(A, B, out=C), reps)
        batch = 1
        for s in sa[:-2]:
            batch *= s
        flops = (8 if pairing == "CC" else 4) * batch * sa[-2] * sa[-1] * sb[-1]
        r = {"pairing": pairing, "A": list(sa), "B": list(sb), "ms": round(ms, 4),
             "TFLOP/s": round(flops / ms / 1e9, 2), "of_peak": round(flops / ms / 1e-3 / PEAK, 3)}
        out.append(r)
        print(json.dumps(r), flush=True)
        del A, B, C
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
