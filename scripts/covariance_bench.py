#!/usr/bin/env python3
"""Timing of mrx_tod_gram on one GPU: `n_groups` groups of `n_det` rows of a [n_groups n_det, T] float32 TOD of
unit white noise, at T = `n_samples` and at n_samples / 8 (the length after downsample(8)), one call per group as
maria_amd.covariance makes them: without flags, with flags (3 % set), and with flags and the counts.  Beside them, in the
same run: a device-to-device copy of the TOD, making the zero-filled centred copy Z that a library product needs
(where(flags, 0, x - mean)), and torch's float32 Z @ Z.T per group.  Medians of `reps` passes after a warm-up; each line
gives the multiply-adds of the symmetric half (R (R + 1) / 2 * T per group) and the rate they amount to, 2 flop each.
The lines go to stdout and to `out` (default profiles/covariance_bench.txt).
Usage: python scripts/covariance_bench.py [n_det] [n_samples] [n_groups] [reps] [out]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from maria_amd._lib import GRAM_BLOCK, Context, ptr  # noqa: E402
from scripts.subscans_bench import median_ms  # noqa: E402


def main():
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
    T_full = int(sys.argv[2]) if len(sys.argv) > 2 else 240000
    n_g = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    out = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "covariance_bench.txt")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    D = n_g * R
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for T in (T_full, T_full // 8):
        x = torch.randn((D, T), dtype=torch.float32, device=dev)
        flags = (torch.rand((D, T), device=dev) < 0.03).to(torch.uint8)
        center = x.double().mean(dim=1)
        rows = [torch.arange(g * R, (g + 1) * R, dtype=torch.int32, device=dev) for g in range(n_g)]
        G = torch.empty((R, R), dtype=torch.float64, device=dev)
        n = torch.empty((R, R), dtype=torch.int32, device=dev)
        macs = n_g * (R * (R + 1) / 2) * T
        say(f"# {n_g} groups of {R} x {T} float32 ({D * T * 4 / 1e9:.2f} GB), MRX_GRAM_BLOCK {GRAM_BLOCK}, medians of {reps} passes; "
            f"the symmetric half is {macs:.3g} multiply-adds")

        def report(name, ms):
            say(f"{name:58s} {ms:10.3f} ms   {2 * macs / ms / 1e9:7.1f} TF of the symmetric half")

        def gram(f, counts):
            for g in range(n_g):
                ctx.call("mrx_tod_gram", ptr(x), T, None, 0, ptr(f), T if f is not None else 0, D, T, ptr(rows[g]), R, ptr(center), ptr(G),
                         ptr(n) if counts else None)

        report("mrx_tod_gram", median_ms(lambda: gram(None, False), reps))
        report("mrx_tod_gram + counts (no flags: a fill)", median_ms(lambda: gram(None, True), reps))
        report("mrx_tod_gram + flags", median_ms(lambda: gram(flags, False), reps))  # noqa: B023
        report("mrx_tod_gram + flags + counts", median_ms(lambda: gram(flags, True), reps))  # noqa: B023
        y = torch.empty_like(x)
        say(f"{'a copy of the TOD':58s} {median_ms(lambda: y.copy_(x), reps):10.3f} ms")  # noqa: B023
        c32 = center.float()[:, None]

        def zero_filled():
            torch.sub(x, c32, out=y)  # noqa: B023
            y.masked_fill_(flags != 0, 0.0)  # noqa: B023

        say(f"{'the zero-filled centred copy Z (torch)':58s} {median_ms(zero_filled, reps):10.3f} ms")
        P = torch.empty((R, R), dtype=torch.float32, device=dev)

        def product():
            for g in range(n_g):
                torch.matmul(y[g * R:(g + 1) * R], y[g * R:(g + 1) * R].T, out=P)  # noqa: B023

        ms = median_ms(product, reps)
        say(f"{'torch float32 Z @ Z.T (the full square)':58s} {ms:10.3f} ms   {4 * macs / ms / 1e9:7.1f} TF of the full square")
        del x, flags, y
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
