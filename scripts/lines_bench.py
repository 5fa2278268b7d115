#!/usr/bin/env python3
"""Timing of mrx_tod_line_normal and mrx_tod_line_apply on one GPU: a [D, T] float32 TOD of unit white noise
cut into S equal chunks, the normal equations at L = 1 and L = 3 lines with n_poly = 2 (K = 4 and 8), without and with
flags (3 % set), mrx_tod_segment_normal at the same K beside each (the same sums over a polynomial basis: what the
carriers cost is the difference), the application out of place and in place, and one lines.fit (normal equations +
regress.solve of D S systems).  Medians of `reps` passes after a warm-up, each beside the bytes the entry has to move
(4 D T of x, + D T of flags; the application 4 D T read + 4 D T written) and the time they take at the rate a
device-to-device copy of the TOD reaches in the same run, which is measured first.  The lines go to stdout and to `out`
(default profiles/lines_bench.txt).
Usage: python scripts/lines_bench.py [n_det] [n_samples] [n_chunks] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import lines  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs]))


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    S = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "lines_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
    y = torch.empty_like(x)
    bounds = torch.as_tensor(np.linspace(0, T, S + 1).round().astype(np.int32)).to(dev)
    copy_ms = median_ms(lambda: y.copy_(x), reps)
    rate = 8.0 * D * T / copy_ms * 1e3  # bytes a second, read + written
    rows = [f"# line removal of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in {S} chunks of {T // S} samples, medians of {reps} passes; "
            f"a copy of the TOD takes {copy_ms:.3f} ms: {rate / 1e12:.2f} TB/s, the rate of every 'floor'"]

    def report(name, ms, nbytes, evals=0):
        floor = nbytes / rate * 1e3
        per = f"   {ms * 1e6 / evals * 1e3:6.2f} ps a (sample, line)" if evals else ""
        rows.append(f"{name:52s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {floor:6.3f} ms ({ms / floor:6.1f} x){per}")
        print(rows[-1], flush=True)

    print(rows[0], flush=True)
    n_poly = 2
    rng = np.random.default_rng(0)
    for L in (1, 3):
        K = n_poly + 2 * L
        nu_host = np.sort(rng.uniform(0.01, 0.49, (D, L)), axis=1)
        nu = torch.as_tensor(nu_host).to(dev)
        N = torch.empty((D, S, K, K), dtype=torch.float64, device=dev)
        r = torch.empty((D, S, K), dtype=torch.float64, device=dev)
        hits = torch.empty((D, S), dtype=torch.int32, device=dev)
        for name, f, nbytes in (("", None, 4.0), (" + flags", flags, 5.0)):
            ld_f = T if f is not None else 0
            ms = median_ms(lambda: ctx.call("mrx_tod_line_normal", ptr(x), T, None, 0, ptr(f), ld_f, D, T, ptr(bounds), S, ptr(nu), L, n_poly,  # noqa: B023
                                            ptr(N), ptr(r), ptr(hits)), reps)  # noqa: B023
            report(f"mrx_tod_line_normal L = {L}, n_poly = 2 (K = {K}){name}", ms, nbytes * D * T, evals=float(D) * T * L)
            ms = median_ms(lambda: ctx.call("mrx_tod_segment_normal", ptr(x), T, None, 0, ptr(f), ld_f, D, T, ptr(bounds), S, K, ptr(N), ptr(r),  # noqa: B023
                                            ptr(hits)), reps)  # noqa: B023
            report(f"mrx_tod_segment_normal K = {K}{name}", ms, nbytes * D * T)
        a = torch.randn((D, S, K), dtype=torch.float64, device=dev)
        for name, dst in (("out of place", y), ("in place", x)):
            ms = median_ms(lambda: ctx.call("mrx_tod_line_apply", ptr(x), T, D, T, ptr(bounds), S, ptr(nu), L, n_poly, ptr(a), -1, ptr(dst), T), reps)  # noqa: B023
            report(f"mrx_tod_line_apply L = {L} {name}", ms, 8.0 * D * T, evals=float(D) * T * L)
        x.normal_()  # the in-place passes drifted it
        ms = median_ms(lambda: lines.fit(x, bounds, nu_host, n_poly=n_poly, flags=flags, ctx=ctx), max(reps // 2, 1))  # noqa: B023
        rows.append(f"{f'lines.fit L = {L}, n_poly = 2 + flags ({D * S} systems)':52s} {ms:9.3f} ms")
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
