"""CPU tier of maria_amd.jumps: the reference's statistic against a double loop, the peak rule on plateaus,
the jump injector's reproducibility, the refusals, which come before any device call, and the recovery conditions of the
reference alone on the data the device tier reuses."""

import jumps_ref as ref
import numpy as np
import pytest
import torch

from maria_amd import jumps

SEEDS = (1, 2, 3)  # of noisy_rows in the recovery tests, here and on the device; the reference passes on each
RECOVERY = dict(D=16, T=3 * 1024 + 17, w=32, n_sigma=8.0, sep=32, gap=4)


def recovery_conditions(truth_pos, truth_height, row_start, pos, height, ok, scale, gap):
    """Assert the four conditions; returns (worst position error, worst height error in robust scales)."""
    D = truth_pos.shape[0]
    worst_p, worst_h = 0, 0.0
    for d in range(D):
        p, h = pos[row_start[d]:row_start[d + 1]], height[row_start[d]:row_start[d + 1]]
        assert len(p) == truth_pos.shape[1], (d, "a jump missed or a peak that is no jump", p, truth_pos[d])
        assert ok[row_start[d]:row_start[d + 1]].all(), d
        dp = np.abs(p.astype(np.int64) - truth_pos[d])
        dh = np.abs(h - truth_height[d]) / scale[d]
        assert dp.max() <= gap, (d, p, truth_pos[d])
        assert dh.max() <= 5.0, (d, h, truth_height[d], scale[d])
        worst_p, worst_h = max(worst_p, int(dp.max())), max(worst_h, float(dh.max()))
    return worst_p, worst_h


@pytest.mark.parametrize("w,g,m", [(2, 0, 1), (5, 2, None), (8, 0, 8), (16, 3, 1)])
def test_reference_statistic_is_the_double_loop(w, g, m):
    rng = np.random.default_rng(w + g)
    for T in (1, 2, w, 2 * w + 1, 61):
        x = (rng.standard_normal((3, T)) * 3 + 5).astype(np.float32)
        f = (rng.random((3, T)) < 0.2).astype(np.uint8)
        f[1] = 1  # a row flagged end to end
        for flags in (None, f):
            s, scale = ref.step_statistic(x, w, g, flags, m)
            want = ref.step_statistic_by_loops(x, w, g, flags, m)
            assert s.dtype == np.float32
            # both are a float64 value rounded to float32; the two float64 values differ by the rounding of sums of
            # <= 61 terms, which can move the float32 rounding by one ulp of s: 2^-23 |s| <= 2^-22 max(|mean_L|, |mean_R|)
            formed = scale > 0
            assert np.all(np.abs(s.astype(np.float64) - want)[formed] <= 2.0**-22 * scale[formed]), (T, flags is None)
            assert not s[~formed].any() and not want[~formed].any()
            if flags is not None:
                assert not s[1].any()
    xi = rng.integers(-64, 65, (2, 61)).astype(np.float32)  # exact sums: equal bit for bit
    assert np.array_equal(ref.step_statistic(xi, w, g, None, m)[0], ref.step_statistic_by_loops(xi, w, g, None, m))


def test_reference_peak_rule_on_plateaus():
    s = np.zeros((1, 60), np.float32)
    s[0, 10:14] = -3.0       # a plateau: its earliest sample
    s[0, 30], s[0, 33] = 2.0, 2.0  # two equal samples within sep: the earlier
    s[0, 50], s[0, 52] = 1.5, 2.5  # a lower one before a higher one within sep: the higher
    f, n = ref.find(s, [1.0], sep=4, grow_before=1, grow_after=2)
    assert np.flatnonzero(f[0] == 1).tolist() == [10, 30, 52] and n[0] == 3
    want = np.zeros(60, np.uint8)
    for p in (10, 30, 52):
        want[p - 1:p + 3] = 2
    want[[10, 30, 52]] = 1
    np.testing.assert_array_equal(f[0], want)
    # sep 2: 33 is now out of 30's reach and a peak of its own; 50 is still under 52
    f, n = ref.find(s, [1.0], sep=2, grow_before=0, grow_after=0)
    assert np.flatnonzero(f[0]).tolist() == [10, 30, 33, 52]
    # a strict threshold, a NaN threshold, a row of zeros at threshold 0
    assert ref.find(s, [3.0], 4, 0, 0)[1][0] == 0 and ref.find(s, [np.nan], 4, 0, 0)[1][0] == 0
    assert ref.find(np.full((1, 20), 0.0, np.float32), [0.0], 4, 0, 0)[1][0] == 0
    c = ref.find(np.full((1, 20), 2.5, np.float32), [0.0], 4, 3, 3)
    assert np.flatnonzero(c[0][0] == 1).tolist() == [0]  # a plateau longer than sep: its earliest sample alone


@pytest.mark.parametrize("sep", [1, 3, 32])
def test_reference_peaks_are_more_than_sep_apart(sep):
    s = ref.quantised_statistic(8, 700, sep)  # a few values: ties and plateaus in every window
    f, n = ref.find(s, np.zeros(8), sep, 0, 0)
    assert n.sum() > 8
    for d in range(8):
        p = np.flatnonzero(f[d] == 1)
        assert len(p) == n[d] and (len(p) < 2 or np.diff(p).min() > sep)


def test_draw_and_inject_jumps_are_reproducible_by_seed():
    a = jumps.draw_jumps(6, 2000, 4, (8.0, 16.0), 11, margin=64, spacing=96)
    b = jumps.draw_jumps(6, 2000, 4, (8.0, 16.0), 11, margin=64, spacing=96)
    c = jumps.draw_jumps(6, 2000, 4, (8.0, 16.0), 12, margin=64, spacing=96)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    pos, h = a
    assert pos.dtype == np.int64 and pos.shape == (6, 4) and h.shape == (6, 4)
    assert pos.min() >= 64 and pos.max() < 2000 - 64 and np.diff(pos, axis=1).min() >= 96
    assert np.all((np.abs(h) >= 8) & (np.abs(h) <= 16)) and (h > 0).any() and (h < 0).any()
    assert np.all((pos[:, :1] - 64) % 96 == (pos - 64) % 96)  # one offset a row
    x = torch.zeros((6, 2000), dtype=torch.float32)
    got = jumps.inject_jumps(x, 4, (8.0, 16.0), 11, margin=64, spacing=96)
    assert np.array_equal(got[0], pos) and np.array_equal(got[1], h)
    want = np.zeros((6, 2000))
    for d in range(6):
        for p, v in zip(pos[d], h[d]):
            want[d, p:] += v
    np.testing.assert_array_equal(x.numpy(), want.astype(np.float32))
    one = jumps.draw_jumps(2, 10, 0, 1.0, 0)
    assert one[0].shape == (2, 0)


def test_cumulative_heights_restart_at_every_row():
    rs = np.array([0, 2, 2, 5], np.int32)
    h = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    np.testing.assert_array_equal(jumps.cumulative_heights(rs, h), [1.0, 3.0, 4.0, 12.0, 28.0])
    np.testing.assert_array_equal(ref.cumulative(rs, h), [1.0, 3.0, 4.0, 12.0, 28.0])


def test_refusals_come_before_any_device_call(monkeypatch):
    """Everything the four entries refuse raises ValueError on the host: no context is made and no entry is called."""
    from maria_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call")

    monkeypatch.setattr(_lib.Context, "__init__", no_device)
    monkeypatch.setattr(_lib.Context, "call", no_device)
    x = torch.zeros((3, 100), dtype=torch.float32)
    f = torch.zeros((3, 100), dtype=torch.uint8)
    rs, ps, h = np.array([0, 1, 1, 2], np.int32), np.array([10, 50], np.int32), np.array([1.0, 2.0])
    shape = {
        "D 0": dict(x=x[:0]),
        "T 0": dict(x=x[:, :0]),
        "1-D x": dict(x=x[0]),
        "float64 x": dict(x=x.double()),
        "numpy x": dict(x=np.zeros((3, 100), np.float32)),
        "strided samples": dict(x=x[:, ::2]),
        "pitch < T": dict(x=torch.as_strided(x, (3, 100), (50, 1))),
        "host x": dict(x=x),  # the last refusal: everything else about this call is in order
    }
    window = {
        "window 1": dict(x=x, window=1), "window 257": dict(x=x, window=257), "window 2.5": dict(x=x, window=2.5),
        "min_count 0": dict(x=x, window=8, min_count=0), "min_count 9": dict(x=x, window=8, min_count=9),
        "min_count 1.5": dict(x=x, window=8, min_count=1.5),
    }
    gap = {"gap -1": dict(x=x, window=8, gap=-1), "gap 65": dict(x=x, window=8, gap=65), "gap 0.5": dict(x=x, window=8, gap=0.5)}
    flags = {
        "flags shape": dict(x=x, window=8, flags=f[:, :99]),
        "flags dtype": dict(x=x, window=8, flags=f.bool()),
        "flags numpy": dict(x=x, window=8, flags=f.numpy()),
        "flags strided": dict(x=x, window=8, flags=torch.zeros((3, 200), dtype=torch.uint8)[:, ::2]),
        "flags pitch": dict(x=x, window=8, flags=torch.as_strided(torch.zeros(300, dtype=torch.uint8), (3, 100), (60, 1))),
    }
    lists = {
        "row_start length": dict(row_start=rs[:-1]), "row_start from 1": dict(row_start=np.array([1, 1, 1, 2])),
        "row_start to 3": dict(row_start=np.array([0, 1, 1, 3])), "row_start decreasing": dict(row_start=np.array([0, 2, 1, 2])),
        "row_start float": dict(row_start=rs.astype(float)), "pos 2-D": dict(pos=ps[None]), "pos float": dict(pos=ps.astype(float)),
        "pos -1": dict(pos=np.array([-1, 50])), "pos T": dict(pos=np.array([10, 100])),
        "pos descending in a row": dict(row_start=np.array([0, 2, 2, 2]), pos=np.array([50, 10])),
    }
    with_window = lambda cases: {k: dict({"window": 8}, **v) for k, v in cases.items()}  # noqa: E731
    cases = {
        jumps.step_statistic: {
            **with_window(shape), **window, **gap, **flags,
            "out is x": dict(x=x, window=8, out=x),
            "out overlaps x": dict(x=x[:2], window=8, out=torch.as_strided(x, (2, 100), (100, 1), 50)),
            "out shape": dict(x=x, window=8, out=torch.zeros((3, 99))),
            "out dtype": dict(x=x, window=8, out=torch.zeros((3, 100), dtype=torch.float64)),
            "out pitch": dict(x=x, window=8, out=torch.as_strided(torch.zeros(300), (3, 100), (60, 1))),
        },
        jumps.find_jumps: {
            **shape, **window, **flags,
            "sep 0": dict(x=x, sep=0), "sep 513": dict(x=x, sep=513), "sep 1.5": dict(x=x, sep=1.5),
            "grow 65": dict(x=x, grow=(65, 0)), "grow -1": dict(x=x, grow=(0, -1)), "grow 1.5": dict(x=x, grow=(1.5, 2)),
            "grow scalar": dict(x=x, grow=3),
            "n_sigma nan": dict(x=x, n_sigma=float("nan")), "n_sigma inf": dict(x=x, n_sigma=float("inf"), sigma=1.0),
            "n_sigma < 0": dict(x=x, n_sigma=-1.0),
            "sigma nan": dict(x=x, sigma=np.array([1.0, np.nan, 1.0])), "sigma inf": dict(x=x, sigma=float("inf")),
            "sigma < 0": dict(x=x, sigma=torch.tensor([1.0, -1.0, 1.0])), "sigma shape": dict(x=x, sigma=np.ones(4)),
            "no scratch": dict(x=x, scratch_bytes=0),
        },
        jumps.jump_heights: {
            **{k: dict(dict(x=x, row_start=rs, pos=ps, window=8, gap=2), **v) for k, v in {**shape, **window, **gap, **flags, **lists}.items()},
        },
        jumps.fix_jumps: {
            **{k: dict(dict(x=x, row_start=rs, pos=ps, height=h), **v) for k, v in {**shape, **lists}.items()},
            "height length": dict(x=x, row_start=rs, pos=ps, height=h[:1]),
            "height nan": dict(x=x, row_start=rs, pos=ps, height=np.array([1.0, np.nan])),
            "out overlaps x": dict(x=x[:2], row_start=rs[:3], pos=ps[:1], height=h[:1], out=torch.as_strided(x, (2, 100), (100, 1), 50)),
            "out shape": dict(x=x, row_start=rs, pos=ps, height=h, out=torch.zeros((3, 99))),
            "out dtype": dict(x=x, row_start=rs, pos=ps, height=h, out=torch.zeros((3, 100), dtype=torch.float64)),
            "out pitch": dict(x=x, row_start=rs, pos=ps, height=h, out=torch.as_strided(torch.zeros(300), (3, 100), (60, 1))),
            "in place on the host": dict(x=x, row_start=rs, pos=ps, height=h, out=x),
        },
    }
    for fn, bad in cases.items():
        for name, kw in bad.items():
            with pytest.raises(ValueError):
                fn(**kw)
                pytest.fail(f"{fn.__name__}: {name}")
    for kw in (dict(s=x[0]), dict(s=x.double()), dict(s=x, scratch_bytes=0), dict(s=x, scratch_bytes=1.5)):
        with pytest.raises(ValueError):
            jumps.robust_scale(**kw)
    for kw in (dict(n_per_row=5, amplitude=1.0, seed=0, margin=10, spacing=20), dict(n_per_row=1, amplitude=-1.0, seed=0),
               dict(n_per_row=1, amplitude=(2.0, 1.0), seed=0), dict(n_per_row=1, amplitude=1.0, seed=0, spacing=0),
               dict(n_per_row=1, amplitude=1.0, seed=0, margin=-1), dict(n_per_row=1.5, amplitude=1.0, seed=0)):
        with pytest.raises(ValueError):
            jumps.inject_jumps(x, **kw)
    assert not x.any()


def test_tod_fix_jumps_refuses_before_any_device_call(monkeypatch):
    from maria_amd import _lib
    from maria_amd.sim import TOD

    def no_device(*a, **k):
        raise AssertionError("a device call")

    monkeypatch.setattr(_lib.Context, "__init__", no_device)
    monkeypatch.setattr(TOD, "_device_fields", no_device)
    tod = TOD({"a": np.zeros((2, 300), np.float32)}, dets=None, coords=None)
    for kw in (dict(window=1), dict(window=300), dict(gap=65), dict(sep=0), dict(sep=600), dict(grow=(0, 65)), dict(min_count=0),
               dict(window=16, min_count=17), dict(n_fit=0), dict(n_fit=17)):
        with pytest.raises(ValueError):
            tod.fix_jumps(**kw)


def test_robust_scale_is_the_lower_median_in_chunks():
    s = torch.as_tensor(np.random.default_rng(5).standard_normal((7, 300)).astype(np.float32))  # an even T
    want = ref.robust_scale(s.numpy())
    for scratch in (1 << 30, 4 * 300 * 3 + 1, 1):  # one chunk, 3 + 3 + 1 rows, a row at a time
        got = jumps.robust_scale(s, scratch_bytes=scratch)
        assert got.dtype == torch.float64
        np.testing.assert_array_equal(got.numpy(), want)


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_recovers_the_jumps_of_noisy_rows(seed):
    """No injected jump missed, no other peak, every position within ``gap`` of the truth, every height within 5 robust
    scales of the statistic (the height estimator is the statistic itself, so its error has that scale)."""
    c = RECOVERY
    x, flags, pos, height = ref.noisy_rows(c["D"], c["T"], c["w"], seed)
    assert 0.015 < flags.mean() < 0.025 and np.diff(pos, axis=1).min() >= 3 * c["w"]
    assert pos.min() >= 2 * c["w"] and pos.max() < c["T"] - 2 * c["w"] and np.abs(height).min() >= 8 and np.abs(height).max() <= 16
    row_start, p, h, ok, scale, _ = ref.recover(x, flags, c["w"], c["n_sigma"], c["sep"], c["gap"])
    worst = recovery_conditions(pos, height, row_start, p, h, ok, scale, c["gap"])
    print(f"seed {seed}: worst position error {worst[0]} samples, worst height error {worst[1]:.2f} robust scales; scale {scale.min():.3f} .. {scale.max():.3f}")
