#!/usr/bin/env python3
"""Timing of mrx_tod_segment_normal and mrx_tod_segment_apply on one GPU: a [D, T] float32 TOD of unit white
noise cut into S equal segments, the normal equations without and with flags (3 % set) at K = 4 and K = 8, the application
out of place and in place, and one subscans.fit (normal equations + regress.solve of D S systems).  Medians of `reps`
passes after a warm-up, each beside the bytes the entry has to move (4 D T of x, + D T of flags; the application 4 D T
read + 4 D T written; the outputs of the reduction left out) and the time they take at the rate a device-to-device copy
of the TOD reaches in the same run, which is measured first.  The lines go to stdout and to `out` (default
profiles/subscans_bench.txt).
Usage: python scripts/subscans_bench.py [n_det] [n_samples] [n_segments] [reps] [out]

With `project` as the first argument: the frozen projector of DESIGN 3.35 instead.  mrx_tod_segment_project forward and
transposed beside the three-call form it replaces (mrx_tod_segment_normal, regress.solve of the D S systems,
mrx_tod_segment_apply in place) and a copy of the TOD, at K = 4 and K = 8, without and with flags (3 % set); medians of
`reps` (default 5) passes, to profiles/subscan_project_bench.txt.  The fused call has to move 4 D T read (+ D T of flags) and
4 D T written; its second read of a segment is counted only if it misses the caches.
Usage: python scripts/subscans_bench.py project [n_det] [n_samples] [n_segments] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import subscans  # noqa: E402
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


def project_main(argv):
    from maria_amd.regress import solve

    D = int(argv[0]) if len(argv) > 0 else 10000
    T = int(argv[1]) if len(argv) > 1 else 240000
    S = int(argv[2]) if len(argv) > 2 else 60
    reps = int(argv[3]) if len(argv) > 3 else 5
    out = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "subscan_project_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
    y = torch.empty_like(x)
    bounds = torch.as_tensor(np.linspace(0, T, S + 1).round().astype(np.int32)).to(dev)
    copy_ms = median_ms(lambda: y.copy_(x), reps)
    del y
    rate = 8.0 * D * T / copy_ms * 1e3
    lines = [f"# frozen subscan projector of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in {S} segments of {T // S} samples, medians of {reps} "
             f"passes; a copy of the TOD takes {copy_ms:.3f} ms: {rate / 1e12:.2f} TB/s, the rate of every 'floor'"]
    print(lines[0], flush=True)

    def report(name, ms, nbytes):
        floor = nbytes / rate * 1e3
        lines.append(f"{name:58s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {floor:6.3f} ms ({ms / floor:6.1f} x)")
        print(lines[-1], flush=True)

    for K in (4, 8):
        for name, f in (("", None), (" + flags", flags)):
            ld_f = T if f is not None else 0
            nbytes = (8.0 + (1.0 if f is not None else 0.0)) * D * T
            N, _, hits = subscans.normal_equations(x, bounds, K, flags=f, ctx=ctx)
            A, ok = subscans.freeze(N, hits)
            r = torch.empty((D, S, K), dtype=torch.float64, device=dev)
            h32 = torch.empty((D, S), dtype=torch.int32, device=dev)
            for word, transpose in (("forward", 0), ("transposed", 1)):
                ms = median_ms(lambda: ctx.call("mrx_tod_segment_project", ptr(x), T, ptr(f), ld_f, D, T, ptr(bounds), S, K, ptr(A), ptr(ok),  # noqa: B023
                                                transpose, None), reps)  # noqa: B023
                report(f"mrx_tod_segment_project K = {K}{name} {word}", ms, nbytes)
                x.normal_()  # the in-place passes drifted it

            def three_calls():
                ctx.call("mrx_tod_segment_normal", ptr(x), T, None, 0, ptr(f), ld_f, D, T, ptr(bounds), S, K, ptr(N), ptr(r), ptr(h32))  # noqa: B023
                a, _ = solve(N.view(D * S, K, K), r.view(D * S, K), h32.view(D * S))  # noqa: B023
                ctx.call("mrx_tod_segment_apply", ptr(x), T, D, T, ptr(bounds), S, K, ptr(a), -1, ptr(x), T)  # noqa: B023

            ms = median_ms(three_calls, reps)
            report(f"segment_normal + solve + segment_apply K = {K}{name}", ms, nbytes + 4.0 * D * T)  # x is read twice
            x.normal_()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "project":
        return project_main(sys.argv[2:])
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    S = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "subscans_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
    y = torch.empty_like(x)
    bounds = torch.as_tensor(np.linspace(0, T, S + 1).round().astype(np.int32)).to(dev)
    copy_ms = median_ms(lambda: y.copy_(x), reps)
    rate = 8.0 * D * T / copy_ms * 1e3  # bytes a second, read + written
    lines = [f"# subscan filter of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in {S} segments of {T // S} samples, medians of {reps} passes; "
             f"a copy of the TOD takes {copy_ms:.3f} ms: {rate / 1e12:.2f} TB/s, the rate of every 'floor'"]

    def report(name, ms, nbytes):
        floor = nbytes / rate * 1e3
        lines.append(f"{name:52s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {floor:6.3f} ms ({ms / floor:6.1f} x)")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    for K in (4, 8):
        N = torch.empty((D, S, K, K), dtype=torch.float64, device=dev)
        r = torch.empty((D, S, K), dtype=torch.float64, device=dev)
        hits = torch.empty((D, S), dtype=torch.int32, device=dev)
        for name, f, nbytes in (("", None, 4.0), (" + flags", flags, 5.0)):
            ms = median_ms(lambda: ctx.call("mrx_tod_segment_normal", ptr(x), T, None, 0, ptr(f), T if f is not None else 0, D, T, ptr(bounds), S, K,  # noqa: B023
                                            ptr(N), ptr(r), ptr(hits)), reps)  # noqa: B023
            report(f"mrx_tod_segment_normal K = {K}{name}", ms, nbytes * D * T)
        a = torch.randn((D, S, K), dtype=torch.float64, device=dev)
        for name, dst in (("out of place", y), ("in place", x)):
            ms = median_ms(lambda: ctx.call("mrx_tod_segment_apply", ptr(x), T, D, T, ptr(bounds), S, K, ptr(a), -1, ptr(dst), T), reps)  # noqa: B023
            report(f"mrx_tod_segment_apply K = {K} {name}", ms, 8.0 * D * T)
        x.normal_()  # the in-place passes drifted it
        ms = median_ms(lambda: subscans.fit(x, bounds, K, flags=flags, ctx=ctx), max(reps // 2, 1))  # noqa: B023
        lines.append(f"{f'subscans.fit K = {K} + flags ({D * S} systems)':52s} {ms:9.3f} ms")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
