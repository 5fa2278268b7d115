#!/usr/bin/env python3
"""Timing of the maximum-likelihood map-maker's operators on one GPU: mrx_map_project, mrx_map_normal_apply
(routed and atomic), the composition it replaces (mrx_map_project then mrx_bin_map_bucketed), mrx_bin_map_blocks and one
whole MaximumLikelihoodMapper.run(), medians of several passes, for nearest / bilinear pointing and S = 1 / 3.
Usage: python scripts/mlmap_bench.py [n_det] [n_samples] [n_map] [reps]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import synthetic  # noqa: E402
from maria_amd._lib import Context, MrxSkyMap, ptr  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

WORK_CAP = 40 << 30


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    t = 1.7e9 + np.arange(T) / 400.0
    az, el = synthetic.daisy_scan(t)
    off = synthetic.hex_pack(D, np.radians(1.0))
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    d_az, d_el, d_dx, d_dy = f32(az), f32(el), f32(off[:, 0]), f32(off[:, 1])
    gamma = np.radians(45.0 * (np.arange(D) % 4))
    m = 0.5 * np.stack([np.ones(D), np.cos(2 * gamma), np.sin(2 * gamma)], axis=1)
    tod = torch.empty((D, T), dtype=torch.float32, device=dev)
    step = 0.05 / n
    print(f"# {D} detectors x {T} samples (daisy scan, 400 Hz) onto {n}^2, medians of {reps} passes (ms)")
    for bil in (0, 1):
        for S in (1, 3):
            d_sw = torch.as_tensor(np.ascontiguousarray(m[:, :S])).to(dev)
            sky = MrxSkyMap(None, 1, S, n, n, 0.025, -step, -0.025, step, float(np.mean(az)), float(np.mean(el)), bil, 0)
            x = torch.randn((S, 1, n, n), dtype=torch.float64, device=dev)
            y = torch.zeros_like(x)
            wgt = torch.zeros_like(x)
            H = torch.zeros((S * (S + 1) // 2, 1, n, n), dtype=torch.float64, device=dev)
            point = (ptr(d_az), ptr(d_el), T, None, ptr(d_dx), ptr(d_dy), ptr(d_sw), None, D)
            lo, full = C.c_size_t(), C.c_size_t()
            ctx.lib.mrx_map_normal_work_bytes(C.byref(sky), D, T, C.byref(lo), C.byref(full))
            work = torch.empty(max(lo.value, min(full.value, WORK_CAP)), dtype=torch.uint8, device=dev)
            project = lambda: ctx.call("mrx_map_project", C.byref(sky), ptr(x), *point, 1.0, 0.0, ptr(tod), tod.stride(0))  # noqa: E731
            fused = lambda: ctx.call("mrx_map_normal_apply", C.byref(sky), ptr(x), None, 0, None, *point, ptr(y), ptr(work), work.numel())  # noqa: E731
            atomic = lambda: ctx.call("mrx_map_normal_apply", C.byref(sky), ptr(x), None, 0, None, *point, ptr(y), None, 0)  # noqa: E731
            binning = lambda: ctx.call("mrx_bin_map_bucketed", C.byref(sky), ptr(tod), tod.stride(0), None, 0, *point, ptr(y), ptr(wgt),  # noqa: E731
                                       ptr(work), work.numel())
            blocks = lambda: ctx.call("mrx_bin_map_blocks", C.byref(sky), None, 0, None, *point, ptr(H))  # noqa: E731
            rows = {"project": timeit(project, reps)[0], "bin_map_bucketed": timeit(binning, reps)[0]}
            rows["composition"] = rows["project"] + rows["bin_map_bucketed"]
            rows["normal_apply (routed)"] = timeit(fused, reps)[0]
            rows["normal_apply (atomic)"] = timeit(atomic, reps)[0]
            rows["bin_map_blocks"] = timeit(blocks, reps)[0]
            name = f"{'bilinear' if bil else 'nearest'} S={S}"
            print(f"{name:14s} " + "  ".join(f"{k} {v:.2f}" for k, v in rows.items()), flush=True)
            del work
            torch.cuda.empty_cache()
    # one whole run(): IQU, nearest (block solve) and bilinear (20 PCG iterations at most), uniform weights
    from maria_amd.instrument import Band, Detectors
    from maria_amd.mappers import MaximumLikelihoodMapper
    from maria_amd.sim import TOD, Coordinates

    dets = Detectors(off, [Band(center=150e9, width=30e9, name="f150")], gamma=gamma)
    torch.randn((D, T), out=tod)
    data = TOD({"map": tod}, dets, Coordinates(t, az, el, offsets=off), units="K_RJ")
    width = np.degrees(n * step)
    for bil in (False, True):
        mapper = MaximumLikelihoodMapper([data], center=(np.degrees(np.mean(az)), np.degrees(np.mean(el))), width=width, resolution=width / n,
                                         frame="az/el", stokes="IQU", bilinear=bil, noise_weights="uniform", max_iter=20, tol=1e-12)
        mapper.run()  # (warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mapper.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"run() IQU {'bilinear' if bil else 'nearest'}: {dt * 1e3:.0f} ms, {mapper.products['n_iter']} PCG iterations")


if __name__ == "__main__":
    main()
