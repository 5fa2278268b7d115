#!/usr/bin/env python3
"""Timing of mrx_tod_column_mean, mrx_tod_regress_normal and mrx_tod_regress_apply on one GPU: a [D, T]
float32 TOD of unit white noise in G = 2 groups of alternating rows, Gaussian templates, the reductions without and with
flags (3 % set), at K = 2 and K = 8; the application out of place and in place; regress.solve; and one
regress.fit_common_mode of three iterations at K = 2.  Medians of `reps` passes after a warm-up, each beside the bytes
the entry has to move (4 D T of x, + D T of flags; the application 4 D T read + 4 D T written; the templates, G K T
floats shared by the rows of a group, and the outputs of the reductions left out) and the time a copy's 6.3 TB/s would
take for them.  The lines go to stdout and to `out` (default profiles/regress_bench.txt).
Usage: python scripts/regress_bench.py [n_det] [n_samples] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import regress  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402

COPY_BYTES_PER_S = 6.3e12
G = 2


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
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "regress_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
    y = torch.empty_like(x)
    group = (torch.arange(D, device=dev) % G).to(torch.int32)
    u = torch.ones(D, dtype=torch.float64, device=dev)
    S = torch.empty((G, T), dtype=torch.float64, device=dev)
    W = torch.empty((G, T), dtype=torch.float64, device=dev)
    mean = torch.empty((G, T), dtype=torch.float32, device=dev)
    lines = [f"# common-mode regression of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in {G} groups, medians of {reps} passes; "
             f"'floor': the bytes at the {COPY_BYTES_PER_S / 1e12:.1f} TB/s of a copy"]

    def report(name, ms, nbytes):
        lines.append(f"{name:52s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {nbytes / COPY_BYTES_PER_S * 1e3:6.3f} ms "
                     f"({ms / (nbytes / COPY_BYTES_PER_S * 1e3):6.1f} x)")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    for name, f, nbytes in (("", None, 4.0), (" + flags", flags, 5.0)):
        ms = median_ms(lambda: ctx.call("mrx_tod_column_mean", ptr(x), T, None, 0, ptr(f), T if f is not None else 0, D, T, ptr(group), G,  # noqa: B023
                                        ptr(u), ptr(u), None, ptr(S), ptr(W), ptr(mean), T), reps)
        report(f"mrx_tod_column_mean{name}", ms, nbytes * D * T)
    for K in (2, 8):
        B = torch.randn((G, K, T), dtype=torch.float32, device=dev)
        N = torch.empty((D, K, K), dtype=torch.float64, device=dev)
        r = torch.empty((D, K), dtype=torch.float64, device=dev)
        hits = torch.empty((D,), dtype=torch.int32, device=dev)
        for name, f, nbytes in (("", None, 4.0), (" + flags", flags, 5.0)):
            ms = median_ms(lambda: ctx.call("mrx_tod_regress_normal", ptr(x), T, None, 0, ptr(f), T if f is not None else 0, D, T, ptr(group), G,  # noqa: B023
                                            ptr(B), T, K, ptr(N), ptr(r), ptr(hits)), reps)  # noqa: B023
            report(f"mrx_tod_regress_normal K = {K}{name}", ms, nbytes * D * T)
        ms = median_ms(lambda: regress.solve(N, r, hits.to(torch.int64)), reps)  # noqa: B023
        lines.append(f"{f'regress.solve K = {K} ({D} rows)':52s} {ms:9.3f} ms")
        print(lines[-1], flush=True)
        a = torch.randn((D, K), dtype=torch.float64, device=dev)
        for name, dst in (("out of place", y), ("in place", x)):
            ms = median_ms(lambda: ctx.call("mrx_tod_regress_apply", ptr(x), T, D, T, ptr(group), G, ptr(B), T, K, ptr(a), -1, ptr(dst), T), reps)  # noqa: B023
            report(f"mrx_tod_regress_apply K = {K} {name}", ms, 8.0 * D * T)
        x.normal_()  # the in-place passes drifted it
    for name, f in (("", None), (" + flags", flags)):
        ms = median_ms(lambda: regress.fit_common_mode(x, groups=group, n_groups=G, flags=f, n_iter=3, ctx=ctx), max(reps // 2, 1))  # noqa: B023
        lines.append(f"{f'regress.fit_common_mode, 3 iterations, K = 2{name}':52s} {ms:9.3f} ms")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
