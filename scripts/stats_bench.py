#!/usr/bin/env python3
"""Timing of mrx_tod_segment_moments and mrx_tod_segment_flag on one GPU: a [D, T] float32 TOD of unit white
noise cut into S equal segments; the moments without and with flags (3 % set) and with a model, the flagging with every
segment masked, one in twenty and none, and beside them mrx_tod_segment_normal at K = 4 (the kernel of the same shape that
evaluates a basis) without and with flags.  Medians of `reps` passes after a warm-up, each beside the bytes the entry
has to move (4 D T of x, + 4 D T of a model, + D T of flags; the flagging reads and writes the flags of the masked
segments alone, 2 D T times their share; the outputs of the reductions left out) and the time they take at the rate a device-to-device copy of the TOD reaches in the same run,
which is measured first.  The lines go to stdout and to `out` (default profiles/stats_bench.txt).
Usage: python scripts/stats_bench.py [n_det] [n_samples] [n_segments] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd._lib import Context, ptr  # noqa: E402
from scripts.subscans_bench import median_ms  # noqa: E402


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    S = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "stats_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
    y = torch.empty_like(x)
    bounds = torch.as_tensor(np.linspace(0, T, S + 1).round().astype(np.int32)).to(dev)
    copy_ms = median_ms(lambda: y.copy_(x), reps)
    rate = 8.0 * D * T / copy_ms * 1e3  # bytes a second, read + written
    lines = [f"# statistics of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in {S} segments of {T // S} samples, medians of {reps} passes; "
             f"a copy of the TOD takes {copy_ms:.3f} ms: {rate / 1e12:.2f} TB/s, the rate of every 'floor'"]

    def report(name, ms, nbytes):
        floor = nbytes / rate * 1e3
        ratio = f"{ms / floor:6.1f} x" if floor > 0 else "nothing to move"
        lines.append(f"{name:52s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {floor:6.3f} ms ({ratio})")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    K = 4
    N = torch.empty((D, S, K, K), dtype=torch.float64, device=dev)
    r = torch.empty((D, S, K), dtype=torch.float64, device=dev)
    hits = torch.empty((D, S), dtype=torch.int32, device=dev)
    stat = torch.empty((D, S, 8), dtype=torch.float64, device=dev)
    count = torch.empty((D, S, 2), dtype=torch.int32, device=dev)
    for name, f, nbytes in (("", None, 4.0), (" + flags", flags, 5.0)):
        ms = median_ms(lambda: ctx.call("mrx_tod_segment_normal", ptr(x), T, None, 0, ptr(f), T if f is not None else 0, D, T, ptr(bounds), S, K,  # noqa: B023
                                        ptr(N), ptr(r), ptr(hits)), reps)  # noqa: B023
        report(f"mrx_tod_segment_normal K = {K}{name}", ms, nbytes * D * T)
    for name, m, f, nbytes in (("", None, None, 4.0), (" + flags", None, flags, 5.0), (" + model + flags", y, flags, 9.0)):
        ms = median_ms(lambda: ctx.call("mrx_tod_segment_moments", ptr(x), T, ptr(m), T if m is not None else 0, ptr(f), T if f is not None else 0,  # noqa: B023
                                        D, T, ptr(bounds), S, ptr(stat), ptr(count)), reps)  # noqa: B023
        report(f"mrx_tod_segment_moments{name}", ms, nbytes * D * T)
    for name, share in (("every segment", 1.0), ("one segment in twenty", 0.05), ("no segment", 0.0)):
        mask = (torch.rand((D, S), device=dev) < share).to(torch.uint8)
        ms = median_ms(lambda: ctx.call("mrx_tod_segment_flag", ptr(flags), T, D, T, ptr(bounds), S, ptr(mask), 4), reps)  # noqa: B023
        report(f"mrx_tod_segment_flag, {name}", ms, 2.0 * float(mask.float().mean()) * D * T)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
