#!/usr/bin/env python3
"""Timing of mrx_tod_column_fit and mrx_tod_column_apply on one GPU: a [D, T] float32 TOD of unit white
noise in G = 2 groups of alternating rows, the basis of random focal-plane positions, at K = 1, 3 and 6 terms, without and
with flags (3 % set); the application out of place and in place; beside a copy of the TOD in the same run.  Medians of
`reps` passes after a warm-up, each beside the bytes the entry has to move (the fit 4 D T of x, + D T of flags; the
application 4 D T read + 4 D T written; the coefficients, G K T doubles shared by the rows of a group, left out) and the
time the run's own copy rate would take for them.  The lines go to stdout and to `out` (default
profiles/skypoly_bench.txt).
Usage: python scripts/skypoly_bench.py [n_det] [n_samples] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from maria_amd import sky_polynomial  # noqa: E402
from maria_amd._lib import Context, ptr  # noqa: E402

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
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "skypoly_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    x = torch.randn((D, T), dtype=torch.float32, device=dev)
    flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
    y = torch.empty_like(x)
    groups = (np.arange(D) % G).astype(np.int32)
    group = torch.as_tensor(groups).to(dev)
    u = torch.ones(D, dtype=torch.float64, device=dev)
    copy_ms = median_ms(lambda: y.copy_(x), reps)
    rate = 8.0 * D * T / copy_ms * 1e3  # bytes a second, read + written
    lines = [f"# sky polynomial of {D} x {T} float32 ({D * T * 4 / 1e9:.1f} GB) in {G} groups, medians of {reps} passes; 'floor': the bytes at "
             f"the {rate / 1e12:.2f} TB/s of this run's copy ({copy_ms:.3f} ms)"]

    def report(name, ms, nbytes):
        floor = nbytes / rate * 1e3
        lines.append(f"{name:52s} {ms:9.3f} ms   {nbytes / 1e9:6.2f} GB  {nbytes / ms / 1e6:7.0f} GB/s   floor {floor:6.3f} ms ({ms / floor:6.1f} x)")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    for order in (0, 1, 2):
        K = sky_polynomial.n_terms(order)
        P = torch.as_tensor(sky_polynomial.basis(np.random.default_rng(order).uniform(-1, 1, (D, 2)), order, groups, G)).to(dev)
        c = torch.empty((G, K, T), dtype=torch.float64, device=dev)
        ok = torch.empty((G, T), dtype=torch.uint8, device=dev)
        for name, f, nbytes in (("", None, 4.0), (" + flags", flags, 5.0)):
            ms = median_ms(lambda: ctx.call("mrx_tod_column_fit", ptr(x), T, None, 0, ptr(f), T if f is not None else 0, D, T, ptr(group), G,  # noqa: B023
                                            ptr(P), K, ptr(u), ptr(u), None, 2 * K, 1e-10, ptr(c), T, ptr(ok), None, None, None), reps)  # noqa: B023
            report(f"mrx_tod_column_fit K = {K}{name}", ms, nbytes * D * T)
        for name, dst in (("out of place", y), ("in place", x)):
            ms = median_ms(lambda: ctx.call("mrx_tod_column_apply", ptr(x), T, D, T, ptr(group), G, ptr(P), K, ptr(c), T, None, ptr(u), -1,  # noqa: B023
                                            ptr(dst), T), reps)  # noqa: B023
            report(f"mrx_tod_column_apply K = {K} {name}", ms, 8.0 * D * T)
        x.normal_()  # the in-place passes drifted it
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
