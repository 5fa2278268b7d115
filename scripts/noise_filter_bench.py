#!/usr/bin/env python3
"""Timing of the correlated-noise GLS map's operators on one GPU: mrx_tod_noise_filter in place on a
[D, T] float32 TOD at several K, against the HBM floor (one read and one write of the TOD at the 6.3 TB/s a copy
reaches), and one conjugate-gradient iteration of MaximumLikelihoodMapper(noise_model=...) onto an n^2 IQU map split
into its three steps: mrx_map_project, the filter (K = 2048), mrx_bin_map_bucketed.  Medians of `reps` passes after a
warm-up.
Usage: python scripts/noise_filter_bench.py [n_det] [n_samples] [n_map] [reps]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import noise_filter, synthetic  # noqa: E402
from maria_amd._lib import Context, MrxSkyMap, ptr  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
WORK_CAP = 40 << 30


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    fs = 400.0
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    tod = torch.randn((D, T), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    floor = 2.0 * D * T * 4 / HBM_BYTES_PER_S * 1e3
    print(f"# mrx_tod_noise_filter of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in place, medians of {reps} passes (ms)")
    for K in (256, 1024, 2048):
        lags = noise_filter.lags(1.0, rng.uniform(0.5, 5.0, D), 1.0, fs, K, device=dev)
        ms = timeit(lambda: noise_filter.apply(ctx, tod, lags, None, out=tod), reps)[0]  # noqa: B023
        print(f"K {K:5d}  {ms:8.3f} ms  {2.0 * D * T * 4 / ms / 1e6:6.0f} GB/s  HBM floor {floor:.2f} ms ({100 * floor / ms:.0f} %)", flush=True)
        tod.copy_(torch.randn_like(tod))

    # one CG iteration onto an n^2 IQU map, nearest pointing
    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t)
    off = synthetic.hex_pack(D, np.radians(1.0))
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    d_az, d_el, d_dx, d_dy = f32(az), f32(el), f32(off[:, 0]), f32(off[:, 1])
    gamma = np.radians(45.0 * (np.arange(D) % 4))
    d_sw = torch.as_tensor(0.5 * np.stack([np.ones(D), np.cos(2 * gamma), np.sin(2 * gamma)], axis=1)).to(dev)
    step = 0.05 / n
    sky = MrxSkyMap(None, 1, 3, n, n, 0.025, -step, -0.025, step, float(np.mean(az)), float(np.mean(el)), 0, 0)
    x = torch.randn((3, 1, n, n), dtype=torch.float64, device=dev)
    y, wgt = torch.zeros_like(x), torch.zeros_like(x)
    point = (ptr(d_az), ptr(d_el), T, None, ptr(d_dx), ptr(d_dy), ptr(d_sw), None, D)
    lo, full = C.c_size_t(), C.c_size_t()
    ctx.lib.mrx_bin_map_work_bytes(C.byref(sky), D, T, C.byref(lo), C.byref(full))
    work = torch.empty(max(lo.value, min(full.value, WORK_CAP)), dtype=torch.uint8, device=dev)
    lags = noise_filter.lags(1.0, rng.uniform(0.5, 5.0, D), 1.0, fs, 2048, device=dev)
    project = lambda: ctx.call("mrx_map_project", C.byref(sky), ptr(x), *point, 1.0, 0.0, ptr(tod), tod.stride(0))  # noqa: E731
    filt = lambda: noise_filter.apply(ctx, tod, lags, None, out=tod)  # noqa: E731
    binning = lambda: ctx.call("mrx_bin_map_bucketed", C.byref(sky), ptr(tod), tod.stride(0), None, 0, *point, ptr(y), ptr(wgt),  # noqa: E731
                               ptr(work), work.numel())
    rows = {"project": timeit(project, reps)[0], "filter K 2048": timeit(filt, reps)[0], "bin_map_bucketed": timeit(binning, reps)[0]}
    total = sum(rows.values())
    print(f"# one CG iteration onto {n}^2 IQU (nearest): " + "  ".join(f"{k} {v:.2f} ms ({100 * v / total:.0f} %)" for k, v in rows.items())
          + f"  total {total:.2f} ms")


if __name__ == "__main__":
    main()
