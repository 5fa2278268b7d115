#!/usr/bin/env python3
"""Timing of the band powers on one GPU at 3 x 2048^2 and 3 x 4096^2: mrx_map_band_powers (auto and cross
form; bins of 200 from l = 100 to the plane's corner, so that every cell off the Nyquist lines but the few below l = 100 is
read and binned: a cell outside the edges is dropped before its modes are loaded) and the float64 torch.fft.rfft2 of
bandpowers.modes, each beside a device copy (dst.copy_(src): one read and one write) of the bytes it reads -- the modes
[3, n, n/2 + 1] complex128 for the kernel (twice that for the cross form), the maps [3, n, n] float64 for the transform.
The functions take turns pass by pass in one process; medians of `reps` passes after a warm-up, device events around each.
mrx_map_band_powers uploads its edges and waits for the copy on every call: that is in its time.
One GPU step, under a time limit of its own:
    timeout -k 10 300 python scripts/bandpower_bench.py [reps]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import _lib  # noqa: E402
from maria_amd import bandpowers as bp  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402


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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    info = ctx.device_info()
    print(f"# {info['name']}, {info['n_cu']} CUs; medians of {reps} alternating passes (ms); GB/s = bytes read / time")
    res = np.radians(1.0 / 60.0)
    edges = bp.bin_edges(100, 200, np.pi * np.sqrt(2) / res)
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in (2048, 4096):
        tqu = torch.randn((3, n, n), dtype=torch.float64, device=dev, generator=gen)
        m1 = bp.modes(tqu, None, res)
        m2 = bp.modes(tqu.flip(0), None, res)
        map_copy, mode_copy = torch.empty_like(tqu), torch.empty_like(m1.a)
        pair, pair_copy = torch.stack([m1.a, m2.a]), torch.empty((2,) + tuple(m1.a.shape), dtype=m1.a.dtype, device=dev)
        need = C.c_size_t()
        _lib.load().mrx_band_power_work_bytes(n, n, len(edges) - 1, C.byref(need))
        work = torch.empty(need.value // 8, dtype=torch.float64, device=dev)
        sums = torch.empty((len(edges) - 1, 8), dtype=torch.float64, device=dev)
        e = edges.ctypes.data_as(C.POINTER(C.c_double))

        def kernel(a, b):
            ctx.call("mrx_map_band_powers", ptr(a), ptr(b), n, n, float(res), e, len(edges) - 1, ptr(sums), ptr(work), need.value)

        fns = [lambda: kernel(m1.a, m1.a), lambda: mode_copy.copy_(m1.a),
               lambda: kernel(m1.a, m2.a), lambda: pair_copy.copy_(pair),
               lambda: torch.fft.rfft2(tqu, dim=(-2, -1)), lambda: map_copy.copy_(tqu)]
        ms = alternate(fns, reps)
        mode_bytes, map_bytes = m1.a.numel() * 16, tqu.numel() * 8
        rows = [("mrx_map_band_powers, auto", mode_bytes), ("copy of the modes", mode_bytes), ("mrx_map_band_powers, cross", 2 * mode_bytes),
                ("copy of both maps' modes", 2 * mode_bytes), ("torch.fft.rfft2, float64", map_bytes), ("copy of the maps", map_bytes)]
        print(f"3 x {n} x {n}, {len(edges) - 1} bins")
        for (name, nbytes), t in zip(rows, ms):
            print(f"  {name:30s} {t:8.3f} ms   {nbytes / 1e6:8.1f} MB   {nbytes / t / 1e6:8.1f} GB/s")


if __name__ == "__main__":
    main()
