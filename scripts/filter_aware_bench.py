#!/usr/bin/env python3
"""Timing of the filter-aware map's operators on one GPU: mrx_sosfilt and mrx_sosfilt_transpose (with
remove_slope, in place: the same bytes) and mrx_tod_detrend_window against its transpose on a [D, T] float32 TOD; the
pre-processing operator F and F^T of tod_processing.PreprocessOperator for F = low + high pass (4 sections) and one
removed mode; and one conjugate-gradient application of MaximumLikelihoodMapper(filter_aware=True) onto an n^2 map
with S = 1 (I) and S = 3 (IQU) planes, split into mrx_map_project, F, W, F^T and mrx_bin_map_bucketed.  Medians of
`reps` passes after a warm-up.
Usage: python scripts/filter_aware_bench.py [n_det] [n_samples] [n_map] [reps]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.signal  # noqa: E402
import torch  # noqa: E402

from maria_amd import synthetic  # noqa: E402
from maria_amd import tod_processing as tp  # noqa: E402
from maria_amd._lib import Context, MrxSkyMap, ptr  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

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
    fresh = lambda: tod.normal_()  # noqa: E731  (repeated filtering of the same buffer decays to denormals)
    gb = 2.0 * D * T * 4 / 1e9
    print(f"# {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in place, medians of {reps} passes (ms; GB/s of one read and one write)")

    sos = np.concatenate([tp.bessel_sos(10.0, fs, 1, "low"), tp.bessel_sos(0.1, fs, 1, "high")], axis=0)
    plan = tp._sos_plan(ctx, sos, D, T, dev)
    rows = {}
    for name, transpose in (("mrx_sosfilt", False), ("mrx_sosfilt_transpose", True)):
        fresh()
        rows[name] = timeit(lambda: tp._sos_run(ctx, plan, tod, True, transpose), reps)[0]  # noqa: B023
    d_w = torch.as_tensor(scipy.signal.windows.hann(T)).to(dev)
    anchors = torch.empty(2 * D + 16, dtype=torch.float64, device=dev)
    fresh()
    rows["mrx_tod_detrend_window"] = timeit(lambda: ctx.call("mrx_tod_detrend_window", ptr(tod), T, D, T, 1, ptr(d_w), ptr(anchors)), reps)[0]
    fresh()
    rows["mrx_tod_detrend_window_transpose"] = timeit(lambda: ctx.call("mrx_tod_detrend_window_transpose", ptr(tod), T, D, T, 1, ptr(d_w)),
                                                      reps)[0]
    for name, ms in rows.items():
        print(f"{name:34s} {ms:8.3f} ms  {gb / ms * 1e3:6.0f} GB/s", flush=True)
    print(f"mrx_sosfilt_transpose / mrx_sosfilt = {rows['mrx_sosfilt_transpose'] / rows['mrx_sosfilt']:.3f}")

    # F = low + high pass and one frozen mode, as an operator
    rng = np.random.default_rng(0)
    op = tp.PreprocessOperator(ctx, dev)
    op.shape = (D, T)
    U = np.linalg.qr(rng.normal(size=(D, 1)))[0]
    op.steps = [("filter", {"plan": plan}),
                ("remove_modes", {"U": torch.as_tensor(U).to(dev), "norms": torch.as_tensor(rng.uniform(0.5, 2.0, D)).to(dev)})]
    fresh()
    f_ms = timeit(lambda: op.apply(tod), reps)[0]
    fresh()
    ft_ms = timeit(lambda: op.apply_transpose(tod), reps)[0]
    print(f"# F = filter (4 sections) + 1 frozen mode:  F {f_ms:.2f} ms   F^T {ft_ms:.2f} ms", flush=True)

    # one CG application onto an n^2 map, nearest pointing
    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t)
    off = synthetic.hex_pack(D, np.radians(1.0))
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    d_az, d_el, d_dx, d_dy = f32(az), f32(el), f32(off[:, 0]), f32(off[:, 1])
    gamma = np.radians(45.0 * (np.arange(D) % 4))
    iqu = 0.5 * np.stack([np.ones(D), np.cos(2 * gamma), np.sin(2 * gamma)], axis=1)
    det_w = torch.as_tensor(rng.uniform(0.5, 2.0, D).astype(np.float32)).to(dev)
    step = 0.05 / n
    for S in (1, 3):
        d_sw = torch.as_tensor(np.ascontiguousarray(iqu[:, :S])).to(dev)
        sky = MrxSkyMap(None, 1, S, n, n, 0.025, -step, -0.025, step, float(np.mean(az)), float(np.mean(el)), 0, 0)
        x = torch.randn((S, 1, n, n), dtype=torch.float64, device=dev)
        y, wgt = torch.zeros_like(x), torch.zeros_like(x)
        point = (ptr(d_az), ptr(d_el), T, None, ptr(d_dx), ptr(d_dy), ptr(d_sw), None, D)
        lo, full = C.c_size_t(), C.c_size_t()
        ctx.lib.mrx_bin_map_work_bytes(C.byref(sky), D, T, C.byref(lo), C.byref(full))
        work = torch.empty(max(lo.value, min(full.value, WORK_CAP)), dtype=torch.uint8, device=dev)
        project = lambda: ctx.call("mrx_map_project", C.byref(sky), ptr(x), *point, 1.0, 0.0, ptr(tod), tod.stride(0))  # noqa: E731, B023
        binning = lambda: ctx.call("mrx_bin_map_bucketed", C.byref(sky), ptr(tod), tod.stride(0), None, 0, *point, ptr(y), ptr(wgt),  # noqa: E731, B023
                                   ptr(work), work.numel())
        parts = {"project": timeit(project, reps)[0]}
        parts["F"] = timeit(lambda: op.apply(tod), reps)[0]
        parts["W"] = timeit(lambda: tod.mul_(det_w[:, None]), reps)[0]
        parts["F^T"] = timeit(lambda: op.apply_transpose(tod), reps)[0]
        project()
        parts["bin_map_bucketed"] = timeit(binning, reps)[0]
        total = sum(parts.values())
        print(f"# one CG application onto {n}^2, S = {S} (nearest): " + "  ".join(f"{k} {v:.2f} ms ({100 * v / total:.0f} %)" for k, v in parts.items())
              + f"  total {total:.2f} ms", flush=True)
        del work, x, y, wgt


if __name__ == "__main__":
    main()
