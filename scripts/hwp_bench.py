#!/usr/bin/env python3
"""Timing of mrx_tod_demodulate on one GPU: a [D, T] float32 TOD demodulated at q = 8 with the 523 taps of
hwp.design_taps(200 Hz, 2 Hz), in one run beside (a) the unfused route the library offered before: the mixing in torch in
float32 (two [D, T] products) and three mrx_tod_decimate calls, and (b) a copy of the TOD.  The three take turns pass by
pass in one process; medians of `reps` passes after a warm-up.  Also the polarisation-only call and mrx_tod_hwp_modulate
in place.  Per entry the bytes it has to move and the float64 FMA rate.
Usage: python scripts/hwp_bench.py [n_det] [n_samples] [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import downsample, hwp  # noqa: E402
from maria_amd._lib import Context  # noqa: E402


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
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    fs, f_hwp, q = 200.0, 2.0, 8
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    h = hwp.design_taps(fs, f_hwp)
    d_h = downsample.upload_taps(h, dev)
    c = hwp.carrier(hwp.HWP(f_hwp).angle(np.arange(T) / fs))
    d_c = torch.as_tensor(c).to(dev)
    cos32, sin32 = d_c[:, 0].float().contiguous(), d_c[:, 1].float().contiguous()
    x = torch.randn((D, T), dtype=torch.float32, device=dev).add_(5.0)
    T_out = downsample.output_length(T, q)
    fused = torch.empty((3, D, T_out), dtype=torch.float32, device=dev)
    pol = torch.empty((2, D, T_out), dtype=torch.float32, device=dev)
    unfused = torch.empty((3, D, T_out), dtype=torch.float32, device=dev)
    mixed = torch.empty((2, D, T), dtype=torch.float32, device=dev)
    copy = torch.empty_like(x)
    print(f"# mrx_tod_demodulate of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB), q = {q}, {h.size} taps; medians of {reps} alternating passes (ms)")

    def demodulate():
        hwp.demodulate(x, d_c, q, h, h, ctx=ctx, out=tuple(fused))

    def mix_then_decimate():
        torch.mul(x, cos32, out=mixed[0])
        torch.mul(x, sin32, out=mixed[1])
        downsample.decimate(x, q, taps=h, ctx=ctx, out=unfused[0], device_taps=d_h)
        downsample.decimate(mixed[0], q, taps=h, ctx=ctx, out=unfused[1], device_taps=d_h)
        downsample.decimate(mixed[1], q, taps=h, ctx=ctx, out=unfused[2], device_taps=d_h)

    def copy_tod():
        copy.copy_(x)

    def polarisation_only():
        hwp.demodulate(x, d_c, q, taps_p=h, ctx=ctx, out=(None, pol[0], pol[1]), want_t=False)

    ms_fused, ms_unfused, ms_copy, ms_pol = alternate([demodulate, mix_then_decimate, copy_tod, polarisation_only], reps)
    fmas = 3.0 * D * T_out * h.size
    read = 4.0 * D * T
    j = torch.arange(T_out, device=dev)
    H = (h.size - 1) // 2
    inner = (j * q >= H) & (j * q < T - H)
    diff = [float((fused[k][:, inner] - unfused[k][:, inner] * (1 if k == 0 else 2)).abs().max()) for k in range(3)]
    print(f"fused      mrx_tod_demodulate (T, Q, U)          {ms_fused:9.3f} ms   {fmas / ms_fused / 1e9:6.2f} T FMA/s (float64)   reads {read / 1e9:.1f} GB")
    print(f"unfused    2 torch products + 3 mrx_tod_decimate {ms_unfused:9.3f} ms   {fmas / ms_unfused / 1e9:6.2f} T FMA/s             moves {6 * read / 1e9:.1f} GB   "
          f"ratio unfused / fused {ms_unfused / ms_fused:5.2f}")
    print(f"copy       of the TOD                            {ms_copy:9.3f} ms   {2 * read / ms_copy / 1e6:6.0f} GB/s")
    print(f"pol. only  mrx_tod_demodulate (Q, U)             {ms_pol:9.3f} ms   {2 * fmas / 3 / ms_pol / 1e9:6.2f} T FMA/s (float64)")
    print(f"max |fused - unfused| in the interior: T {diff[0]:.2e} (the same sums), Q {diff[1]:.2e}, U {diff[2]:.2e} (the unfused products are float32)")
    (ms_mod,) = alternate([lambda: hwp.modulate(x, mixed[0], mixed[1], d_c, out=x, ctx=ctx)], reps)
    print(f"modulate   mrx_tod_hwp_modulate in place         {ms_mod:9.3f} ms   {4 * read / ms_mod / 1e6:6.0f} GB/s on 16 D T bytes")


if __name__ == "__main__":
    main()
