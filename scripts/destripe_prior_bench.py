#!/usr/bin/env python3
"""Timing of the destriper's baseline prior on one GPU: mrx_baseline_prior_apply, mrx_baseline_band_factor
and mrx_baseline_band_solve, with their achieved bandwidths, and one whole CG iteration of DestripingMapper with and
without the prior (the apply in place of hits * a, the band solve in place of 1 / hits); medians of several passes,
nearest pointing, S = 1 / 3, 16- and 50-sample baselines, the prior of alpha = 1 at a 400 Hz sample rate.
Usage: python scripts/destripe_prior_bench.py [n_det] [n_samples] [n_map] [reps] [band]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import destripe_prior, synthetic  # noqa: E402
from maria_amd._lib import Context, MrxSkyMap, ptr  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

WORK_CAP = 40 << 30


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    band = int(sys.argv[5]) if len(sys.argv) > 5 else 16
    fs = 400.0
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t)
    off = synthetic.hex_pack(D, np.radians(1.0))
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    d_az, d_el, d_dx, d_dy = f32(az), f32(el), f32(off[:, 0]), f32(off[:, 1])
    gamma = np.radians(45.0 * (np.arange(D) % 4))
    m = np.stack([np.ones(D), np.cos(2 * gamma), np.sin(2 * gamma)], axis=1)
    step = 0.05 / n
    print(f"# {D} detectors x {T} samples (daisy scan, {fs:.0f} Hz) onto {n}^2, nearest pixel, prior alpha = 1, band {band}, "
          f"medians of {reps} passes (ms; GB/s of the bytes each kernel must move)")
    for S in (1, 3):
        d_sw = torch.as_tensor(np.ascontiguousarray(m[:, :S])).to(dev)
        sky = MrxSkyMap(None, 1, S, n, n, 0.025, -step, -0.025, step, float(np.mean(az)), float(np.mean(el)), 0, 0)
        point = (ptr(d_az), ptr(d_el), T, None, ptr(d_dx), ptr(d_dy), ptr(d_sw), None, D)
        H = torch.zeros((S * (S + 1) // 2, 1, n, n), dtype=torch.float64, device=dev)
        ctx.call("mrx_bin_map_blocks", C.byref(sky), None, 0, None, *point, ptr(H))
        x = torch.randn((S, 1, n, n), dtype=torch.float64, device=dev)
        y, u = torch.zeros_like(x), torch.zeros_like(x)
        mask = torch.empty((1, n, n), dtype=torch.uint8, device=dev)
        ctx.call("mrx_map_block_solve", S, 1, n * n, ptr(H), ptr(x), 1e-3, 0, ptr(u), ptr(mask))
        lo, full = C.c_size_t(), C.c_size_t()
        ctx.lib.mrx_map_normal_work_bytes(C.byref(sky), D, T, C.byref(lo), C.byref(full))
        work = torch.empty(max(lo.value, min(full.value, WORK_CAP)), dtype=torch.uint8, device=dev)
        for L in (16, 50):
            nb = -(-T // L)
            w = destripe_prior.prior_weights(fs, L, 1.0, nb)
            Kp = destripe_prior.band_lags(w, band)
            d_w = torch.as_tensor(w).to(dev)
            scale = torch.full((D,), 1.0 / 0.1, dtype=torch.float64, device=dev)  # W = 1, knee 0.1 Hz
            a = torch.randn((D, nb), dtype=torch.float64, device=dev)
            r, hits, out = torch.zeros_like(a), torch.zeros_like(a), torch.empty_like(a)
            ctx.call("mrx_baseline_reduce", C.byref(sky), None, 0, None, 0.0, None, 0, None, ptr(mask), L, *point, None, ptr(hits))
            inv_hits = torch.where(hits > 0, 1.0 / hits, torch.zeros_like(hits))
            factor = torch.empty(D * nb * (Kp + 1), dtype=torch.float64, device=dev)
            ok = torch.empty(D, dtype=torch.uint8, device=dev)

            def apply():
                ctx.call("mrx_baseline_prior_apply", D, nb, len(w), ptr(d_w), ptr(scale), ptr(hits), ptr(a), ptr(out))

            def factorize():
                ctx.call("mrx_baseline_band_factor", D, nb, Kp, ptr(d_w), ptr(scale), ptr(hits), ptr(factor), ptr(ok))

            def band_solve():
                ctx.call("mrx_baseline_band_solve", D, nb, Kp, ptr(factor), ptr(ok), ptr(a), ptr(out))

            def cg_iteration(with_prior):  # DestripingMapper's apply() and the CG's vector updates
                y.zero_()
                ctx.call("mrx_bin_map_baselines", C.byref(sky), ptr(a), L, None, 0, None, *point, ptr(y), ptr(work), work.numel())
                ctx.call("mrx_map_block_solve", S, 1, n * n, ptr(H), ptr(y), 1e-3, 0, ptr(u), None)
                if with_prior:
                    Aa = torch.empty_like(a)
                    ctx.call("mrx_baseline_prior_apply", D, nb, len(w), ptr(d_w), ptr(scale), ptr(hits), ptr(a), ptr(Aa))
                else:
                    Aa = hits * a
                ctx.call("mrx_baseline_reduce", C.byref(sky), None, 0, ptr(u), 1.0, None, 0, None, ptr(mask), L, *point, ptr(Aa), None)
                alpha = 1.0 / float(torch.sum(a * Aa))
                rr = r - alpha * Aa
                if with_prior:
                    z = torch.empty_like(rr)
                    ctx.call("mrx_baseline_band_solve", D, nb, Kp, ptr(factor), ptr(ok), ptr(rr), ptr(z))
                else:
                    z = inv_hits * rr
                float(torch.sum(rr * z)), float(torch.linalg.vector_norm(rr))

            factorize()
            torch.cuda.synchronize()
            n_ok = int(ok.sum())
            t_apply, t_factor, t_solve = timeit(apply, reps)[0], timeit(factorize, 2)[0], timeit(band_solve, reps)[0]
            gbs = lambda nbytes, ms: nbytes / ms / 1e6  # noqa: E731
            size = D * nb
            print(f"S={S} L={L:<3d} nb={nb} K={len(w)} Kp={Kp} ok={n_ok}/{D}  apply {t_apply:.2f} ({gbs(24 * size, t_apply):.0f} GB/s)  "
                  f"factor {t_factor:.2f} ({gbs(8 * size * (Kp + 2), t_factor):.0f} GB/s)  "
                  f"solve {t_solve:.2f} ({gbs(8 * size * (2 * (Kp + 1) + 4), t_solve):.0f} GB/s)  "
                  f"CG iteration plain {timeit(lambda: cg_iteration(False), reps)[0]:.2f}  prior {timeit(lambda: cg_iteration(True), reps)[0]:.2f}",
                  flush=True)
            del factor, ok, a, r, hits, out, inv_hits
            torch.cuda.empty_cache()
        del work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
