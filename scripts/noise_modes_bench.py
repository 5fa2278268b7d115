#!/usr/bin/env python3
"""Timing of the mode-aware GLS map's pieces on one GPU, on a [D, T] float32 TOD:
- mrx_tod_mode_project at m 1 / 5 / 10 / 16 against its HBM floor (one read of the TOD at 6.3 TB/s);
- mrx_tod_noise_filter_modes in place at K 256 / 2048 and m 0 / 5 / 10 / 16 against mrx_tod_noise_filter;
- the inner solve (m 10): its time and iterations per application;
- one conjugate-gradient iteration of MaximumLikelihoodMapper(noise_model=..., modes) onto an n^2 IQU map split into its
  steps (project, A' x, U^T z, the inner solve, A' (x - U b), binning);
- the mode fit (m 10): the noise-law fits, the Gram, its eigenvectors, the series and the refits.
Medians of `reps` passes after a warm-up.
Usage: python scripts/noise_modes_bench.py [n_det] [n_samples] [n_map] [reps]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import noise_estimate, noise_filter, noise_modes, synthetic  # noqa: E402
from maria_amd._lib import Context, MrxSkyMap, ptr  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
WORK_CAP = 40 << 30


def smooth_coupling(off, m, scale):
    """m smooth focal-plane patterns (low-order products of the offsets), [D, m] float64"""
    u = off[:, 0] / np.abs(off[:, 0]).max()
    v = off[:, 1] / np.abs(off[:, 1]).max()
    cols = [u ** i * v ** j for i in range(6) for j in range(6 - i)]
    return scale * np.stack(cols[:m], axis=1)


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    fs = 400.0
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    rng = np.random.default_rng(0)
    off = synthetic.hex_pack(D, np.radians(1.0))
    tod = torch.randn((D, T), dtype=torch.float32, device=dev)

    floor = D * T * 4 / HBM_BYTES_PER_S * 1e3
    print(f"# mrx_tod_mode_project of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB), medians of {reps} passes (ms)")
    for m in (1, 5, 10, 16):
        U = torch.as_tensor(smooth_coupling(off, m, 1.0)).to(dev).contiguous()
        a = torch.empty((m, T), dtype=torch.float64, device=dev)
        ms = timeit(lambda: noise_modes.project(ctx, tod, U, out=a), reps)[0]  # noqa: B023
        print(f"m {m:2d}  {ms:8.3f} ms  {D * T * 4 / ms / 1e6:6.0f} GB/s  HBM floor {floor:.2f} ms ({100 * floor / ms:.0f} %)", flush=True)

    print("# mrx_tod_noise_filter_modes in place against mrx_tod_noise_filter (ms)")
    for K in (256, 2048):
        lag = noise_filter.lags(1.0, rng.uniform(0.5, 5.0, D), 1.0, fs, K, device=dev)
        base = timeit(lambda: noise_filter.apply(ctx, tod, lag, None, out=tod), reps)[0]  # noqa: B023
        row = [f"K {K:5d}  plain {base:8.3f}"]
        for m in (0, 5, 10, 16):
            U = torch.as_tensor(smooth_coupling(off, max(m, 1), 1.0)).to(dev).contiguous()
            b = torch.randn((max(m, 1), T), dtype=torch.float32, device=dev)
            ms = timeit(lambda: ctx.call("mrx_tod_noise_filter_modes", ptr(tod), T, ptr(tod), T, D, T, ptr(lag), K, None, 0,  # noqa: B023
                                         ptr(U), m, ptr(b)), reps)[0]
            row.append(f"m {m:2d} {ms:8.3f} ({100 * (ms / base - 1):+.0f} %)")
        print("  ".join(row), flush=True)
        tod.copy_(torch.randn_like(tod))

    # the inner solve, m 10, K 2048, a 1/f law per detector and per mode
    m, K = 10, 2048
    lag = noise_filter.lags(1.0, rng.uniform(0.5, 5.0, D), 1.0, fs, K, device=dev).contiguous()
    U = torch.as_tensor(smooth_coupling(off, m, 0.3)).to(dev).contiguous()
    beta = noise_filter.lags(np.full(m, 1e-2), np.full(m, 2.0), np.full(m, 1.5), fs, K, device=dev).contiguous()
    t0 = time.perf_counter()
    model = noise_modes.ModeModel(U, beta, lag, None, T, noise_modes.inner_tol(1e-8))
    torch.cuda.synchronize()
    setup = 1e3 * (time.perf_counter() - t0)
    z = noise_filter.apply(ctx, tod, lag, None)
    a = noise_modes.project(ctx, z, U)
    ms = timeit(lambda: model.inner.solve(a, model.tol), reps)[0]
    its = model.inner.iterations[-reps:]
    print(f"# inner solve, m {m}, K {K}, tol {model.tol:.0e}: {ms:.2f} ms, {its[-1]} iterations ({ms / max(its[-1], 1):.3f} ms each); "
          f"set-up (G lags, spectra, preconditioner) {setup:.1f} ms")

    # one CG iteration onto an n^2 IQU map, nearest pointing, m 10
    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t)
    f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float32)).to(dev)  # noqa: E731
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
    scratch = torch.empty_like(tod)
    state = {}

    def step_a():
        noise_filter.apply(ctx, tod, lag, None, out=scratch)

    def step_b():
        state["a"] = noise_modes.project(ctx, scratch, U)

    def step_c():
        state["b"] = model.inner.solve(state["a"], model.tol).float().contiguous()

    def step_d():
        noise_modes.filter_modes(ctx, tod, lag, None, U, state["b"], tod)

    rows = {
        "project": timeit(lambda: ctx.call("mrx_map_project", C.byref(sky), ptr(x), *point, 1.0, 0.0, ptr(tod), tod.stride(0)), reps)[0],
        "A' x": timeit(step_a, reps)[0],
        "U^T z": timeit(step_b, reps)[0],
        "inner solve": timeit(step_c, reps)[0],
        "A' (x - U b)": timeit(step_d, reps)[0],
        "bin_map_bucketed": timeit(lambda: ctx.call("mrx_bin_map_bucketed", C.byref(sky), ptr(tod), tod.stride(0), None, 0, *point, ptr(y),
                                                    ptr(wgt), ptr(work), work.numel()), reps)[0],
    }
    total = sum(rows.values())
    print(f"# one CG iteration onto {n}^2 IQU (nearest), m {m}, K {K}: "
          + "  ".join(f"{k} {v:.2f} ms ({100 * v / total:.0f} %)" for k, v in rows.items()) + f"  total {total:.2f} ms", flush=True)
    del scratch, work

    # the fit, m 10, on a TOD with 10 shared 1/f modes
    tod.normal_()
    common = torch.cumsum(torch.randn((m, T), dtype=torch.float32, device=dev), dim=1) * 0.01
    tod.addmm_(U.float(), common)
    fit_law = lambda rows: noise_estimate.fit_noise(*noise_estimate.welch(rows, fs, ctx=ctx))  # noqa: E731
    noise_modes.fit(ctx, tod[:64, : min(T, 65536)].contiguous(), 4, fit_law)  # warm-up of the shapes' libraries
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    law0 = fit_law(tod)
    torch.cuda.synchronize()
    t_law = time.perf_counter() - t0
    t0 = time.perf_counter()
    fitted = noise_modes.fit(ctx, tod, m, fit_law)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    del law0
    print(f"# mode fit, m {m}, {D} x {T}: {t_fit:.2f} s (one noise-law fit of every row: {t_law:.2f} s; the fit makes three); "
          f"{fitted['modes'].shape[1]} modes kept, dropped {fitted['dropped'].tolist()}")


if __name__ == "__main__":
    main()
