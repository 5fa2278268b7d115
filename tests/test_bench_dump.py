"""bench.py --dump-outputs (CPU tier): the sample of the last timed step's outputs is a function of the shapes
alone, stays within 64 MB of float32 / float64 at the benchmark's own sizes, and is written as DIR/<name>.npy."""

from __future__ import annotations

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _bytes(D, T, sizes):
    rows, cols, pixels = bench.dump_selection(D, T, sizes)
    n_cols = T if cols is None else len(cols)
    return 4 * len(rows) * n_cols + 8 * len(rows) + (0 if cols is None else 8 * len(cols)) + 4 * sum(len(p) for p in pixels)


@pytest.mark.parametrize("D,T,sizes", [
    (10000, 240000, [2048 * 2048] * 8),      # atlast_10k on one GPU
    (6250, 1440000, [4096 * 4096] * 16),     # atlast_50k, one GPU's share
    (2, 20_000_000, [64 * 64]),              # a row longer than the TOD budget: samples are sampled too
    (3, 100, [16 * 16, 8 * 8]),              # smaller than the budget: everything, pixels up to the smallest screen
])
def test_selection_is_seeded_sorted_and_within_the_limit(D, T, sizes):
    a, b = bench.dump_selection(D, T, sizes), bench.dump_selection(D, T, sizes)
    for x, y in zip(a[:2], b[:2]):
        assert (x is None and y is None) or np.array_equal(x, y)
    assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2]))
    rows, cols, pixels = a
    assert len(rows) >= 1 and np.all(np.diff(rows) > 0) and rows[-1] < D
    if cols is not None:
        assert np.all(np.diff(cols) > 0) and cols[-1] < T
    assert len({len(p) for p in pixels}) == 1
    for p, n in zip(pixels, sizes):
        assert len(p) >= 1 and np.all(np.diff(p) > 0) and p[-1] < n
    assert _bytes(D, T, sizes) <= bench.DUMP_MAX_BYTES


def test_small_outputs_are_kept_whole():
    rows, cols, pixels = bench.dump_selection(3, 100, [256, 64])
    assert list(rows) == [0, 1, 2] and cols is None and [len(p) for p in pixels] == [64, 64]


def test_dump_writes_float_arrays(tmp_path):
    import torch

    g = torch.Generator().manual_seed(0)
    tod = torch.randn(40, 300, generator=g)
    screens = [torch.randn(32, 32, generator=g), torch.randn(16, 48, generator=g)]
    out = tmp_path / "dump"
    shapes = bench.dump_outputs(str(out), tod, screens, row_offset=1000)
    assert sorted(os.listdir(out)) == ["screens.npy", "tod.npy", "tod_rows.npy"]
    got = {n: np.load(out / f"{n}.npy") for n in shapes}
    assert {n: list(a.shape) for n, a in got.items()} == shapes
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    rows = got["tod_rows"].astype(np.int64) - 1000
    assert np.array_equal(got["tod"], tod.numpy()[rows])
    _, _, pixels = bench.dump_selection(40, 300, [1024, 768])
    for k, (s, p) in enumerate(zip(screens, pixels)):
        assert np.array_equal(got["screens"][k], s.numpy().reshape(-1)[p])
    # the same inputs, the same files
    bench.dump_outputs(str(tmp_path / "again"), tod, screens, row_offset=1000)
    for n in shapes:
        assert np.array_equal(np.load(tmp_path / "again" / f"{n}.npy"), got[n])


def test_steps_and_dump_arguments():
    args = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "d"])
    assert args.steps == 7 and args.warmup == 0 and args.dump_outputs == "d"
    assert bench.parse_args([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    args = bench.parse_args(["--steps", "7", "--warmup", "0", "--full", "--no-frontend"])
    assert args.full and args.no_frontend and args.steps == 7 and args.warmup == 0
