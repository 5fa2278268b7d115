#!/usr/bin/env python3
"""Timing of mrx_tod_onepole and mrx_tod_onepole_inverse on one GPU: a [D, T] float32 TOD of unit white
noise, every row with a time constant of 1 .. 10 ms at 400 Hz, the lag and its inverse out of place and in place.  Medians
of `reps` passes after a warm-up, each beside the bytes the entry has to move (4 D T read + 4 D T written) and the time
they take at the rate a device-to-device copy of the TOD reaches in the same run, which is measured first.  The lines go
to stdout and to `out` (default profiles/timeconst_bench.txt).
Usage: python scripts/timeconst_bench.py [n_det] [n_samples] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import time_constants  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs]))


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "timeconst_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    a = torch.as_tensor(time_constants.poles(np.random.default_rng(0).uniform(1e-3, 10e-3, D), 400.0)).to(dev)
    copy_ms = median_ms(lambda: y.copy_(x), reps)
    rate = 8.0 * D * T / copy_ms * 1e3  # bytes a second, read + written
    lines = [f"# detector time constants of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB), poles {float(a.min()):.3f} .. {float(a.max()):.3f}, "
             f"medians of {reps} passes; a copy of the TOD takes {copy_ms:.3f} ms: {rate / 1e12:.2f} TB/s, the rate of every 'floor'"]
    print(lines[0], flush=True)
    nbytes = 8.0 * D * T
    for entry in ("mrx_tod_onepole", "mrx_tod_onepole_inverse"):
        for name, dst in (("out of place", y), ("in place", x)):
            ms = median_ms(lambda: ctx.call(entry, ptr(x), T, D, T, ptr(a), 1, ptr(dst), T), reps)  # noqa: B023
            floor = nbytes / rate * 1e3
            lines.append(f"{entry + ' ' + name:40s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {floor:6.3f} ms ({ms / floor:6.2f} x)")
            print(lines[-1], flush=True)
            x.normal_()  # the in-place passes changed it
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
