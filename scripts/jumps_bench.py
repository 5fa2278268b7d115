#!/usr/bin/env python3
"""Timing of mrx_tod_step_stat, mrx_tod_jump_find, mrx_tod_jump_height and mrx_tod_jump_fix on one GPU: a
[D, T] float32 TOD of unit white noise with 4 jumps a row (8 - 16 sigma of either sign, at least 3 x 256 samples apart),
windows 16, 64 and 256 (gap 4, sep = window, thresholds at 8 robust scales of the statistic, grow (4, 4)), without flags
and with 2 % of the samples flagged at random.  Medians of `reps` passes after a warm-up, each beside the bytes the entry
has to move (statistic: 4 D T read + 4 D T written, + D T of flags; finder: 4 D T read + D T written; fix: 4 D T read +
4 D T written; the heights read 2 window samples a jump) and the time a copy's 6.3 TB/s would take for them.  The lines
go to stdout and to `out` (default profiles/jumps_bench.txt).
Usage: python scripts/jumps_bench.py [n_det] [n_samples] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import jumps  # noqa: E402
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
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "jumps_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    y = torch.zeros_like(x)
    pos, height = jumps.draw_jumps(D, T, 4, (8.0, 16.0), 1, margin=2 * jumps.MAX_WINDOW, spacing=3 * jumps.MAX_WINDOW)
    rows = torch.as_tensor(np.repeat(np.arange(D), 4)).to(dev)
    y[rows, torch.as_tensor(pos.reshape(-1)).to(dev)] = torch.as_tensor(height.reshape(-1).astype(np.float32)).to(dev)
    x += torch.cumsum(y, dim=1)  # the steps, summed in float32: good enough for a timing
    flags = (torch.rand((D, T), device=dev) < 0.02).to(torch.uint8)
    s = y  # the statistic lives where the steps were
    jump_flags = torch.empty((D, T), dtype=torch.uint8, device=dev)
    count = torch.empty(D, dtype=torch.int32, device=dev)
    lines = [f"# jump repair of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB), 4 jumps a row, medians of {reps} passes; "
             f"'floor': the bytes at the {COPY_BYTES_PER_S / 1e12:.1f} TB/s of a copy"]

    def report(name, ms, nbytes, extra=""):
        lines.append(f"{name:44s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {nbytes / COPY_BYTES_PER_S * 1e3:6.3f} ms "
                     f"({ms / (nbytes / COPY_BYTES_PER_S * 1e3):6.1f} x){extra}")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    for w in (16, 64, 256):
        for name, f in (("", None), (", flags", flags)):
            ms = median_ms(lambda: jumps.step_statistic(x, w, 0, flags=f, ctx=ctx, out=s), reps)  # noqa: B023
            report(f"w {w:3d}  mrx_tod_step_stat{name}", ms, (8.0 + (f is not None)) * D * T)
            thresh = (8.0 * jumps.robust_scale(s)).float().contiguous()
            ms = median_ms(lambda: ctx.call("mrx_tod_jump_find", ptr(s), T, D, T, ptr(thresh), w, 4, 4, ptr(jump_flags), T, ptr(count)), reps)  # noqa: B023
            n = int(count.sum())
            report(f"w {w:3d}  mrx_tod_jump_find{name}", ms, 5.0 * D * T, f"   {n} peaks ({n / D:.2f} a row)")
            at = torch.nonzero(jump_flags == 1)
            row_start = torch.zeros(D + 1, dtype=torch.int32, device=dev)
            row_start[1:] = torch.cumsum(count.to(torch.int64), 0).to(torch.int32)
            p = at[:, 1].to(torch.int32).contiguous()
            h = torch.empty(n, dtype=torch.float64, device=dev)
            ok = torch.empty(n, dtype=torch.uint8, device=dev)
            ms = median_ms(lambda: ctx.call("mrx_tod_jump_height", ptr(x), T, ptr(f), T if f is not None else 0, D, T, ptr(row_start), ptr(p), n,  # noqa: B023
                                            w, 4, w // 2, ptr(h), ptr(ok)), reps)  # noqa: B023
            report(f"w {w:3d}  mrx_tod_jump_height{name}", ms, (8.0 + 2 * (f is not None)) * w * n, f"   {n} jumps, {int(ok.sum())} with a height")
    cum = torch.as_tensor(jumps.cumulative_heights(row_start.cpu().numpy(), h.cpu().numpy())).to(dev)
    out_of_place = torch.empty_like(x)
    ms = median_ms(lambda: ctx.call("mrx_tod_jump_fix", ptr(x), T, D, T, ptr(row_start), ptr(p), ptr(cum), n, ptr(out_of_place), T), reps)
    report("mrx_tod_jump_fix, out of place", ms, 8.0 * D * T, f"   {n} jumps")
    zero = torch.zeros_like(cum)  # in place, with heights of 0: every pass sees the same data
    ms = median_ms(lambda: ctx.call("mrx_tod_jump_fix", ptr(x), T, D, T, ptr(row_start), ptr(p), ptr(zero), n, ptr(x), T), reps)
    report("mrx_tod_jump_fix, in place", ms, 8.0 * D * T, f"   {n} jumps")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
