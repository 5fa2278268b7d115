#!/usr/bin/env python3
"""Timing of mrx_tod_decimate on one GPU: a [D, T] float32 TOD decimated by q = 4 / 8 / 16 with the default
taps (20 q + 1), beside what the library could do for the same interior before: mrx_tod_noise_filter with K = H and the
taps as lags (out of place), followed by a [:, ::q] copy.  The two forms alternate pass by pass in one process; medians of
`reps` passes after a warm-up.  Per q: the share of 8 TB/s reached on the 4 D T (1 + 1 / q) bytes the decimator has to
move, its float64 FMA rate (D T_out n_taps FMAs), and the largest difference of the two forms' interiors.
Usage: python scripts/decimate_bench.py [n_det] [n_samples] [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import downsample, noise_filter  # noqa: E402
from maria_amd._lib import Context  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12


def alternate(fns, reps):
    """Medians (ms) of ``reps`` passes of each function, the functions taking turns."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
    for row in evs:
        for fn, (a, b) in zip(fns, row):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [float(np.median([row[i][0].elapsed_time(row[i][1]) for row in evs])) for i in range(len(fns))]


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev).add_(5.0)
    full = torch.empty_like(x)
    print(f"# mrx_tod_decimate of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) against mrx_tod_noise_filter (K = H) + [:, ::q] copy, "
          f"medians of {reps} alternating passes (ms)")
    for q in (4, 8, 16):
        h = downsample.design_taps(q)
        H = (h.size - 1) // 2
        T_out = downsample.output_length(T, q)
        y = torch.empty((D, T_out), dtype=torch.float32, device=dev)
        picked = torch.empty_like(y)
        lags = torch.as_tensor(h[H:]).to(dev).expand(D, -1).contiguous()

        def decimate():
            downsample.decimate(x, q, taps=h, ctx=ctx, out=y)  # noqa: B023

        def filter_then_pick():
            noise_filter.apply(ctx, x, lags, None, out=full)  # noqa: B023
            picked.copy_(full[:, ::q])  # noqa: B023

        ms_dec, ms_ref = alternate([decimate, filter_then_pick], reps)
        j = torch.arange(T_out, device=dev)
        inner = (j * q >= H) & (j * q < T - H)
        diff = float((y[:, inner] - picked[:, inner]).abs().max())
        nbytes = 4.0 * D * T * (1.0 + 1.0 / q)
        fmas = float(D) * T_out * h.size
        print(f"q {q:2d}  taps {h.size:4d}  decimate {ms_dec:8.3f} ms  {nbytes / ms_dec / 1e6:6.0f} GB/s ({100 * nbytes / ms_dec / 1e-3 / HBM_PEAK_BYTES_PER_S:4.1f} % "
              f"of 8 TB/s)  {fmas / ms_dec / 1e9:6.2f} T FMA/s (float64)   filter + pick {ms_ref:8.3f} ms  ratio {ms_ref / ms_dec:5.2f}   "
              f"max |difference| in the interior {diff:.2e}", flush=True)
        del y, picked, lags


if __name__ == "__main__":
    main()
