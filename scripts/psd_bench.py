#!/usr/bin/env python3
"""Timing of the noise estimate on one GPU: mrx_tod_welch at each segment length, with its achieved
bandwidth and its share of the two floors (the row read once at the 6.3 TB/s a copy reaches; 5 n log2 n flop per pair of
segments, 5 log2 n flop a sample, at the 157 TF/s float32 vector peak), and what noise_weights="fit" adds to a
destriper run: the weights' step (Welch at the default segment length, then the fit) against "inverse_variance"'s
variance of every row.  Medians of `reps` passes after a warm-up.
Usage: python scripts/psd_bench.py [n_det] [n_samples] [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import noise_estimate  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
FP32_FLOP_PER_S = 157.3e12


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    fs = 400.0
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    print(f"# mrx_tod_welch of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB), medians of {reps} passes after a warm-up (ms)")
    for n in (256, 1024, 4096, 8192):
        psd = torch.empty((D, n // 2 + 1), dtype=torch.float32, device=dev)

        def run():
            ctx.call("mrx_tod_welch", ptr(x), x.stride(0), D, T, n, fs, ptr(psd))

        ms = timeit(run, reps)[0]
        nseg = (T - n) // (n // 2) + 1
        used = (nseg - 1) * (n // 2) + n  # samples read a row
        nbytes = D * used * 4.0 + psd.numel() * 4.0
        flop = D * ((nseg + 1) // 2) * 5.0 * n * np.log2(n)
        t_hbm, t_fp = nbytes / HBM_BYTES_PER_S * 1e3, flop / FP32_FLOP_PER_S * 1e3
        print(f"nperseg {n:5d}  {ms:7.3f} ms  {nbytes / ms / 1e6:6.0f} GB/s  HBM floor {t_hbm:.2f} ms ({100 * t_hbm / ms:.0f} %)  "
              f"FFT flop floor {t_fp:.2f} ms ({100 * t_fp / ms:.0f} %)", flush=True)
        del psd
    # the destriper's per-detector weights of one TOD: what "fit" adds over "inverse_variance"
    t = np.arange(T) / fs

    def white():
        f, p = noise_estimate.welch(x, fs, ctx=ctx)
        return noise_estimate.fit_noise(f, p)["sigma"]

    def inverse_variance():
        return x.double().var(dim=1)

    n_def = noise_estimate.default_nperseg(T)
    ms_w, ms_v = timeit(white, reps)[0], timeit(inverse_variance, reps)[0]
    ms_welch = timeit(lambda: noise_estimate.welch(x, fs, ctx=ctx), reps)[0]
    print(f"destriper weights of one {D} x {T} TOD ({t[-1]:.0f} s at {fs:.0f} Hz): noise_weights='fit' {ms_w:.1f} ms "
          f"(Welch at nperseg {n_def} {ms_welch:.1f} ms, fit {ms_w - ms_welch:.1f} ms), 'inverse_variance' {ms_v:.1f} ms: "
          f"{ms_w - ms_v:+.1f} ms a run", flush=True)


if __name__ == "__main__":
    main()
