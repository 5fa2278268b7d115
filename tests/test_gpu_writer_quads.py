"""GPU tests of the fused TOD writer's row loop (mrx_spline_upsample_fused, maria_amd/csrc/mrx_spline_tile.h): where the
four samples of every thread of a wave lie in ONE knot interval, a row costs the thread one coefficient read instead of
four (the same nest on the same operands).  MRX_OPT_WRITER_GENERAL = 1 keeps the read per sample everywhere: every case
runs both ways and every word of the two outputs is compared (padding included), and each is held to scipy's
not-a-knot cubic at the writer's tolerance, 2e-7 of the peak.

The shape is the smallest that still has interior tiles, end tiles and two row batches with a ragged one: 70 rows (no
multiple of 32), 256 knots on a 0.125-s grid from 128 s (binary fractions: a sample that sits on a knot computes its
interval exactly), 10 240 samples at a ratio of 40 (ten time tiles).  Which quads share an interval is worked out here
with the kernel's own rule, floor((t - ta0) / dta) clamped to the intervals, and asserted per case: a case that is meant
to take the one-read loop (or not to) does."""

import functools

import numpy as np
import pytest
import scipy.interpolate

pytestmark = pytest.mark.gpu

D, TA = 70, 256
TA0, DTA = 128.0, 0.125
Y = (20 + np.cumsum(np.random.default_rng(14).standard_normal((D, TA)), axis=1) * 0.05).astype(np.float32)


def _grid(T, ratio=40, start=TA0):
    return start + np.arange(T) * (DTA / ratio)


@functools.lru_cache(maxsize=None)
def _cubic(ta0):
    """scipy's cubic through the rows of Y on the knots ta0 + i dta (built once per coarse grid)."""
    return scipy.interpolate.interp1d(ta0 + DTA * np.arange(TA), Y.astype(np.float64), kind="cubic", bounds_error=False,
                                      fill_value="extrapolate", axis=-1)


def _straddling(t, ta0):
    """Per quad of four consecutive samples: do they lie in more than one (clamped) interval?"""
    j = np.clip(np.floor((t - ta0) * (1.0 / DTA)), 0, TA - 2).astype(np.int64)
    q = j[: len(j) // 4 * 4].reshape(-1, 4)
    return (q != q[:, :1]).any(axis=1)


def _wave_has_straddle(t, ta0):
    """Per wave of the writer (64 threads x 4 samples of one 1024-sample tile)."""
    s = _straddling(t, ta0)
    s = np.r_[s, np.zeros(-len(s) % 64, bool)]
    return s.reshape(-1, 64).any(axis=1)


def _run_both(gpu_ctx, t, ta0=TA0, scale=None, rows=None, pad=0):
    """The writer with MRX_OPT_WRITER_GENERAL 0 and 1 on the same inputs: the two [D][T + pad] outputs (numpy)."""
    import torch

    from maria_amd import _lib
    from maria_amd._lib import ptr

    dev = "cuda:0"
    T = len(t)
    ld = T + pad
    d_y = torch.as_tensor(np.ascontiguousarray(Y.T)).to(dev)
    d_t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
    d_scale = None if scale is None else torch.as_tensor(scale).to(dev)
    d_rows = None if rows is None else torch.as_tensor(rows).to(dev)
    outs = []
    try:
        for general in (0, 1):
            gpu_ctx.set_option(_lib.OPT_WRITER_GENERAL, general)
            out = torch.full((D, ld), -7.0, dtype=torch.float32, device=dev)
            gpu_ctx.call("mrx_spline_upsample_fused", ptr(d_y), D, TA, float(ta0), DTA, ptr(d_t), T,
                         None if d_scale is None else ptr(d_scale), None if d_rows is None else ptr(d_rows), ptr(out), ld)
            torch.cuda.synchronize()
            outs.append(out)
    finally:
        gpu_ctx.set_option(_lib.OPT_WRITER_GENERAL, 0)
    assert torch.equal(outs[0], outs[1]), "the one-read row loop and the general one differ"
    return outs[0].cpu().numpy()


def _check(gpu_ctx, t, ta0=TA0, scale=None, rows=None, pad=0):
    out = _run_both(gpu_ctx, t, ta0, scale, rows, pad)
    T = len(t)
    assert (out[:, T:] == -7.0).all(), "wrote past T"
    ref = _cubic(float(ta0))(t)
    if scale is not None:
        ref = ref * scale.astype(np.float64)[:, None]
    got = out[:, :T]
    if rows is not None:
        got = got[rows]  # row d of the input lands in row rows[d]
    err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"MEASURED writer vs scipy: {err:.3e}")
    assert err <= 2e-7


def test_aligned_ratio_40(gpu_ctx):
    """No quad straddles a knot: every wave of every tile, interior and end, takes the one-read loop."""
    t = _grid(10240)
    assert not _straddling(t, TA0).any()
    _check(gpu_ctx, t)


@pytest.mark.parametrize("what", ["scale", "rows", "pitch"])
def test_aligned_with_scale_rows_and_pitch(gpu_ctx, what):
    t = _grid(10240)
    rng = np.random.default_rng(5)
    if what == "scale":
        _check(gpu_ctx, t, scale=rng.uniform(0.5, 2.0, D).astype(np.float32))
    elif what == "rows":
        _check(gpu_ctx, t, rows=rng.permutation(D).astype(np.int32))
    else:
        _check(gpu_ctx, t, pad=4)


def test_odd_pitch_takes_the_scalar_stores(gpu_ctx):
    """ld = T + 3: rows are not 16-byte aligned, no vector store and so no one-read loop."""
    _check(gpu_ctx, _grid(10240), pad=3)


def test_last_quad_not_full(gpu_ctx):
    """T = 10 238 in rows of 10 240 floats: the last thread owns two samples and stores them one by one; every other
    thread's quad is full."""
    t = _grid(10238)
    assert not _straddling(t, TA0).any()
    _check(gpu_ctx, t, pad=2)


def test_ratio_10_quads_straddle(gpu_ctx):
    """Knots every 10 samples: two quads in five hold a knot, in every wave."""
    t = _grid(2560, ratio=10)
    assert _wave_has_straddle(t, TA0).all()
    _check(gpu_ctx, t)


def test_knots_inside_the_quads(gpu_ctx):
    """Ratio 40 with the coarse grid starting at t[2]: every knot falls inside a quad, every wave stays general."""
    t = _grid(10240)
    ta0 = float(t[2])
    assert _wave_has_straddle(t, ta0).all()
    _check(gpu_ctx, t, ta0=ta0)


def test_fast_and_general_waves_in_one_launch(gpu_ctx):
    """Aligned in the first half of t, two samples late in the second: the waves of the first five tiles take the
    one-read loop, those of the last five the general one."""
    t = _grid(10240)
    t[5120:] += 2 * (DTA / 40)
    w = _wave_has_straddle(t, TA0)
    assert not w[:20].any() and w[20:].all()
    _check(gpu_ctx, t)


def test_unsorted_samples_across_a_knot(gpu_ctx):
    """Two samples swapped across a knot (t[2039] and t[2040], the knot at sample 2040): the quad 2036..2039 holds a
    sample of the next interval -- the test on the clamped intervals of all four sends its wave through the general
    loop; its neighbours are untouched."""
    t = _grid(10240)
    t[[2039, 2040]] = t[[2040, 2039]]
    s = _straddling(t, TA0)
    assert s[2036 // 4] and s[2040 // 4] and s.sum() == 2
    _check(gpu_ctx, t)


@pytest.mark.parametrize("ratio", [8, 3])
def test_small_ratios(gpu_ctx, ratio):
    """Ratio 8: the 256-knot image; ratio 3: a tile walked in segments."""
    _check(gpu_ctx, _grid(TA * ratio, ratio=ratio))


def test_samples_outside_the_knots(gpu_ctx):
    """One interval before the first knot and one and a half past the last (the reference extrapolates the end
    cubics): the clamped intervals are equal within each quad there, so those waves take the one-read loop too."""
    t = _grid(40 + 40 * (TA - 1) + 60, start=TA0 - DTA)
    assert not _straddling(t, TA0).any()
    _check(gpu_ctx, t)
