#!/usr/bin/env python3
"""Timing of mrx_cmb_generate on one GPU: T, Q, U of a 2048^2 patch (3 x 2048^2 float32) from the toy
spectrum, in one run beside mrx_screen_generate_batch of three unsmoothed 2048^2 screens -- the same two transform passes
over three planes without the CMB's pass 0.  The two take turns pass by pass in one process; medians of `reps` passes
after a warm-up.  mrx_cmb_generate uploads its coefficient table and waits for the copy on every call: that is in its time.
One GPU step, under a time limit of its own:
    timeout -k 10 120 python scripts/cmb_bench.py [side] [reps]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import _lib, cmb  # noqa: E402
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    res = np.radians(1.0 / 60.0)
    table = cmb.spectrum_table(cmb.toy_spectrum(int(np.pi * np.sqrt(2) / res) + 2, r=0.05), n * res, n * res)
    need = C.c_size_t()
    _lib.load().mrx_cmb_work_floats(n, n, len(table), C.byref(need))
    out = torch.empty((3, n, n), dtype=torch.float32, device=dev)
    work = torch.empty(need.value, dtype=torch.float32, device=dev)
    descs = (_lib.MrxScreenDesc * 3)()
    for k, d in enumerate(descs):
        d.d_out, d.stream, d.dy, d.dx, d.r0, d.nu = out[k].data_ptr(), k, 5.0, 5.0, 300.0, 5.0 / 6.0

    def patch():
        ctx.call("mrx_cmb_generate", 1, 0, n, n, float(res), table.ctypes.data_as(C.c_void_p), len(table), descs, ptr(work), work.numel())

    def screens():
        ctx.call("mrx_screen_generate_batch", 1, n, n, descs, 3, ptr(work), work.numel())

    ms_cmb, ms_scr = alternate([patch, screens], reps)
    print(f"# {n} x {n}, {len(table)} table rows; medians of {reps} alternating passes (ms)")
    print(f"mrx_cmb_generate           T, Q, U            {ms_cmb:8.3f} ms")
    print(f"mrx_screen_generate_batch  3 screens, no beam {ms_scr:8.3f} ms   ratio cmb / screens {ms_cmb / ms_scr:5.2f}")


if __name__ == "__main__":
    main()
