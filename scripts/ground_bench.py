#!/usr/bin/env python3
"""Timing of mrx_tod_bin_reduce and mrx_tod_bin_apply on one GPU: a [D, T] float32 TOD of unit white noise
under the 360 azimuth bins of a daisy scan (synthetic.daisy_scan at 200 Hz), the reduction without and with flags (3 %
set) and a model, the application out of place and in place, and the reduction again under a key in random order (no two
neighbouring samples in one bin: the gather at its worst).  Medians of `reps` passes after a warm-up, each beside the
bytes the entry has to move (reduction: 4 D T of x, + D T of flags, + 4 D T of a model, the lists and the [D, K] outputs
left out; application: 4 D T read + 4 D T written) and the time a copy's 6.3 TB/s would take for them.  The lines go to
stdout and to `out` (default profiles/ground_bench.txt).
Usage: python scripts/ground_bench.py [n_det] [n_samples] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import ground, synthetic  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402

COPY_BYTES_PER_S = 6.3e12
N_BINS = 360


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
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "ground_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    model = torch.randn((D, T), dtype=torch.float32, device=dev)
    flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
    y = torch.empty_like(x)
    az, _ = synthetic.daisy_scan(1.7e9 + np.arange(T) / 200.0, radius_deg=0.5)
    scan, _, _ = ground.azimuth_bins(az, N_BINS)
    run = float(np.mean(np.diff(np.flatnonzero(np.diff(scan) != 0)))) if np.any(np.diff(scan) != 0) else float(T)
    shuffled = np.random.default_rng(0).permutation(T).astype(np.int32) % N_BINS
    sums = torch.empty((D, N_BINS), dtype=torch.float64, device=dev)
    hits = torch.empty((D, N_BINS), dtype=torch.int32, device=dev)
    template = torch.empty((D, N_BINS), dtype=torch.float32, device=dev)
    lines = [f"# azimuth templates of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in {N_BINS} bins (a daisy scan: {run:.1f} consecutive samples "
             f"a visit of a bin), medians of {reps} passes; 'floor': the bytes at the {COPY_BYTES_PER_S / 1e12:.1f} TB/s of a copy"]

    def report(name, ms, nbytes):
        lines.append(f"{name:52s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {nbytes / COPY_BYTES_PER_S * 1e3:6.3f} ms "
                     f"({ms / (nbytes / COPY_BYTES_PER_S * 1e3):6.1f} x)")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    for key_name, key in (("scan", scan), ("random order", shuffled)):
        order, start = ground.bin_lists(key, N_BINS)
        d_order, d_start = torch.as_tensor(order).to(dev), torch.as_tensor(start).to(dev)
        for name, m, f, nbytes in (("", None, None, 4.0), (" + flags", None, flags, 5.0), (" + flags + model", model, flags, 9.0)):
            if key_name != "scan" and m is not None:
                continue

            def reduce():
                ctx.call("mrx_tod_bin_reduce", ptr(x), T, ptr(m), T if m is not None else 0, ptr(f), T if f is not None else 0, D, T,  # noqa: B023
                         ptr(d_order), int(order.size), ptr(d_start), N_BINS, 8, ptr(sums), ptr(hits), ptr(template))  # noqa: B023

            report(f"mrx_tod_bin_reduce{name} ({key_name})", median_ms(reduce, reps), nbytes * D * T)
    order, start = ground.bin_lists(scan, N_BINS)  # the scan's template again: the application subtracts it
    d_order, d_start = torch.as_tensor(order).to(dev), torch.as_tensor(start).to(dev)
    ctx.call("mrx_tod_bin_reduce", ptr(x), T, None, 0, None, 0, D, T, ptr(d_order), int(order.size), ptr(d_start), N_BINS, 8, None, None,
             ptr(template))
    d_bin = torch.as_tensor(scan).to(dev)
    for name, dst in (("out of place", y), ("in place", x)):
        ms = median_ms(lambda: ctx.call("mrx_tod_bin_apply", ptr(x), T, D, T, ptr(d_bin), ptr(template), N_BINS, -1, ptr(dst), T), reps)  # noqa: B023
        report(f"mrx_tod_bin_apply {name} (scan)", ms, 8.0 * D * T)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
