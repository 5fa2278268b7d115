#!/usr/bin/env python3
"""Timing of mrx_tod_source_flag and mrx_tod_beam_normal on one GPU: a [D, T] float32 TOD of a daisy scan over
a point source at the frame's centre plus unit white noise, a hexagonal array, the ra/dec frame.  The source mask at the
default window (3 beam FWHM); the Gauss-Newton sums at K = 5 and K = 7 with that window as flags (a few per cent of the
samples kept: the expectation is about one read of the flags) and with nothing flagged (every sample takes the float64
work).  Medians of `reps` passes after a warm-up, each beside the bytes the entry has to move (the flags once; where
everything is kept also 4 D T of x) and the time they take at the rate a device-to-device copy of the TOD reaches in the
same run; a copy of the flags (read and written) is timed too.  The lines go to stdout and to `out` (default
profiles/beamfit_bench.txt).
Usage: python scripts/beamfit_bench.py [n_det] [n_samples] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import beamfit, synthetic  # noqa: E402
from maria_amd._lib import Context  # noqa: E402
from maria_amd.sim import sky_transform_stack  # noqa: E402
from scripts.subscans_bench import median_ms  # noqa: E402


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "beamfit_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    t = 1.7e9 + np.arange(T) / 50.0
    az, el = synthetic.daisy_scan(t, radius_deg=1.0, speed_deg_s=0.5)
    stack = sky_transform_stack(t, -23.0, -67.8)
    center = beamfit.scan_center(az, el, stack)
    off = synthetic.hex_pack(D, np.radians(1.0))
    fwhm = np.radians(0.17)  # a window of 0.51 degrees: a few per cent of a daisy of 1 degree over an array of 1 degree
    w0 = 8.0 * np.log(2.0) / fwhm**2
    point = {"az": torch.as_tensor(az.astype(np.float32)).to(dev), "el": torch.as_tensor(el.astype(np.float32)).to(dev),
             "transform": torch.as_tensor(stack.reshape(-1, 9)).to(dev), "dx": torch.as_tensor(off[:, 0].astype(np.float32)).to(dev),
             "dy": torch.as_tensor(off[:, 1].astype(np.float32)).to(dev)}
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    copy_ms = median_ms(lambda: y.copy_(x), reps)
    rate = 8.0 * D * T / copy_ms * 1e3  # bytes a second, read + written
    del y
    window = torch.zeros((D, T), dtype=torch.uint8, device=dev)
    beamfit.source_flags(point, center, 3.0 * fwhm, inside=False, flags=window, ctx=ctx)
    kept = 1.0 - float((window != 0).sum()) / (D * T)
    lines = [f"# beam fit of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB), daisy of 1 degree over an array of 1 degree, window 3 x {np.degrees(fwhm):.3f} "
             f"degrees: {100 * kept:.2f} % of the samples kept; medians of {reps} passes; a copy of the TOD takes {copy_ms:.3f} ms: "
             f"{rate / 1e12:.2f} TB/s, the rate of every 'floor'"]

    def report(name, ms, nbytes):
        floor = nbytes / rate * 1e3
        lines.append(f"{name:58s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {floor:6.3f} ms ({ms / floor:6.1f} x)")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    f2 = torch.empty_like(window)
    report("copy of the flags (read + written)", median_ms(lambda: f2.copy_(window), reps), 2.0 * D * T)
    del f2
    scratch = torch.zeros((D, T), dtype=torch.uint8, device=dev)
    report("mrx_tod_source_flag, inside the window (few writes)", median_ms(lambda: beamfit.source_flags(point, center, 3.0 * fwhm, flags=scratch, ctx=ctx), reps),
           1.0 * D * T * kept * 2.0)
    report("mrx_tod_source_flag, outside the window (all written)",
           median_ms(lambda: beamfit.source_flags(point, center, 3.0 * fwhm, inside=False, flags=scratch, ctx=ctx), reps), 2.0 * D * T)
    del scratch
    for K in (5, 7):
        shape = [w0] if K == 5 else [w0, 0.0, w0]
        params = torch.as_tensor(np.concatenate([np.ones((D, 1)), off, np.tile(shape, (D, 1)), np.zeros((D, 1))], axis=1)).to(dev)
        for name, f, nbytes in ((f"window as flags ({100 * kept:.1f} % kept)", window, 1.0 + 4.0 * kept), ("nothing flagged", None, 4.0)):
            ms = median_ms(lambda: beamfit.normal_equations(x, point, center, params, flags=f, ctx=ctx), reps)  # noqa: B023
            report(f"mrx_tod_beam_normal K = {K}, {name}", ms, nbytes * D * T)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
