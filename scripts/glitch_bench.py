#!/usr/bin/env python3
"""Timing of mrx_tod_median_residual, mrx_tod_glitch_flag and mrx_tod_gap_fill on one GPU: a [D, T] float32
TOD of unit white noise with 24 glitches a row (20 - 200 sigma, tau = 3 samples), half windows 5 and 15, thresholds at
6 robust sigmas, grow (2, 8), n_fit 4.  Medians of `reps` passes after a warm-up, each beside the bytes the entry has to
move (residual: 4 D T read + 4 D T written; flag: 4 D T read + D T written; fill: D T of flags read, the few samples it
reads and writes left out) and the time a copy's 6.3 TB/s would take for them, and beside the (2 h + 1)^2 window reads a
sample the rank count makes.  The lines go to stdout and to `out` (default profiles/glitch_bench.txt).
Usage: python scripts/glitch_bench.py [n_det] [n_samples] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import flagging  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402

COPY_BYTES_PER_S = 6.3e12


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
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "glitch_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    flagging.inject_glitches(x, 24, (20.0, 200.0), 3.0, seed=1)
    r = torch.empty_like(x)
    flags = torch.empty((D, T), dtype=torch.uint8, device=dev)
    count = torch.empty(D, dtype=torch.int32, device=dev)
    lines = [f"# glitch flagging of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB), 24 glitches a row, medians of {reps} passes; "
             f"'floor': the bytes at the {COPY_BYTES_PER_S / 1e12:.1f} TB/s of a copy"]

    def report(name, ms, nbytes, extra=""):
        lines.append(f"{name:34s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {nbytes / COPY_BYTES_PER_S * 1e3:6.3f} ms "
                     f"({ms / (nbytes / COPY_BYTES_PER_S * 1e3):6.1f} x){extra}")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    for h in (5, 15):
        sigma = flagging.robust_sigma(x, h, ctx=ctx)
        thresh = (6.0 * sigma).float().contiguous()
        reads = float(D) * T * (2 * h + 1) ** 2

        def residual():
            flagging.median_residual(x, h, ctx=ctx, out=r)  # noqa: B023

        def flag():
            ctx.call("mrx_tod_glitch_flag", ptr(x), T, D, T, h, ptr(thresh), 2, 8, ptr(flags), T, ptr(count))  # noqa: B023

        ms = median_ms(residual, reps)
        report(f"h {h:2d}  mrx_tod_median_residual", ms, 8.0 * D * T, f"   {reads / ms / 1e9:6.2f} T window reads/s")
        ms = median_ms(flag, reps)
        fraction = float(count.sum()) / (D * T)
        report(f"h {h:2d}  mrx_tod_glitch_flag", ms, 5.0 * D * T, f"   {reads / ms / 1e9:6.2f} T window reads/s   flagged {fraction:.3%}")
        r.copy_(x)  # the fill works on a copy: the next half window sees the glitches again
        ms = median_ms(lambda: ctx.call("mrx_tod_gap_fill", ptr(r), T, D, T, ptr(flags), T, 4, ptr(count)), reps)
        report(f"h {h:2d}  mrx_tod_gap_fill (its flags)", ms, 1.0 * D * T, f"   filled {float(count.sum()) / (D * T):.3%}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
