"""maria_amd.downsample on the host: the default taps, the output length, the identity between the direct
formula of mrx_tod_decimate and scipy's resample_poly, and the refusals, which come before any device call."""

import numpy as np
import pytest
import scipy.signal
import torch

from maria_amd import downsample

# the shapes of the GPU tier (tests/test_gpu_downsample.py): (T, q, n_taps)
SHAPES = [(1, 2, 1), (37, 2, 41), (100, 16, 321), (1000, 4, 81), (1025, 3, 1), (4001, 5, 33), (999, 8, 161), (5000, 4, 81)]


def direct(x, q, h):
    """The formula of include/mrx.h in float64: a correlation, out-of-row taps dropped, the rest renormalised."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    H, T = (h.size - 1) // 2, x.shape[-1]
    num = np.zeros(x.shape[:-1] + (downsample.output_length(T, q),))
    den = np.zeros(num.shape[-1])
    for j in range(num.shape[-1]):
        lo, hi = max(0, H - j * q), min(h.size - 1, H + T - 1 - j * q)
        num[..., j] = x[..., j * q + lo - H:j * q + hi - H + 1] @ h[lo:hi + 1]
        den[j] = h[lo:hi + 1].sum()
    return num / den, den


@pytest.mark.parametrize("q", [2, 8, 32])
def test_default_taps_are_scipys_decimate_fir(q):
    h = downsample.design_taps(q)
    ref = scipy.signal.firwin(20 * q + 1, 1.0 / q, window="hamming")  # scipy.signal.decimate(x, q, ftype="fir")
    assert h.dtype == np.float64 and h.shape == (20 * q + 1,)
    np.testing.assert_array_equal(h, ref)
    # ... which is the filter decimate applies: a unit impulse in the interior comes back as the taps at stride q
    x = np.zeros(40 * q + 1)
    x[20 * q] = 1.0
    np.testing.assert_allclose(scipy.signal.decimate(x, q, ftype="fir"), np.pad(h, (10 * q, 10 * q))[::q], atol=1e-15)


def test_output_length():
    for T in (1, 2, 3, 31, 32, 33, 240000, 240001):
        for q in (2, 3, 8, 32):
            assert downsample.output_length(T, q) == len(range(0, T, q)) == -(-T // q)


@pytest.mark.parametrize("T,q,n_taps", SHAPES)
def test_the_formula_is_a_ratio_of_two_resample_poly_calls(T, q, n_taps):
    """Symmetric taps: resample_poly(x, 1, q, window=h) over the same call on ones; general taps: window=h[::-1]."""
    rng = np.random.default_rng(T + q)
    x = rng.standard_normal((2, T)) + 5
    sym = scipy.signal.firwin(n_taps, 1.0 / q) if n_taps > 1 else np.ones(1)
    asym = rng.uniform(0.1, 1.0, n_taps)
    for h, window in ((sym, sym), (asym, asym[::-1])):
        got, den = direct(x, q, h)
        num = scipy.signal.resample_poly(x, 1, q, axis=-1, window=window)
        ones = scipy.signal.resample_poly(np.ones(T), 1, q, window=window)
        assert got.shape == num.shape == (2, -(-T // q))
        # resample_poly scales its window by the up factor (1) only: the ratio is free of any gain convention
        np.testing.assert_allclose(got, num / ones, rtol=1e-13, atol=0)
        np.testing.assert_allclose(den, downsample.truncated_sums(h, T, q), rtol=1e-13, atol=0)


def test_refusals_come_before_any_device_call(monkeypatch):
    """Everything mrx_tod_decimate refuses raises ValueError on the host: no context is made and no entry is called."""
    from maria_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call")

    monkeypatch.setattr(_lib.Context, "__init__", no_device)
    monkeypatch.setattr(_lib.Context, "call", no_device)
    x = torch.zeros((3, 100), dtype=torch.float32)
    h = downsample.design_taps(4)
    bad = {
        "q 1": dict(x=x, q=1),
        "q 33": dict(x=x, q=33),
        "q 2.5": dict(x=x, q=2.5),
        "q 1 with taps": dict(x=x, q=1, taps=h),
        "even taps": dict(x=x, q=4, taps=np.ones(4)),
        "no taps": dict(x=x, q=4, taps=np.ones(0)),
        "1027 taps": dict(x=x, q=4, taps=np.ones(1027)),
        "2-D taps": dict(x=x, q=4, taps=np.ones((3, 3))),
        "NaN tap": dict(x=x, q=4, taps=np.array([1.0, np.nan, 1.0])),
        "D 0": dict(x=x[:0], q=4),
        "T 0": dict(x=x[:, :0], q=4),
        "1-D x": dict(x=x[0], q=4),
        "float64 x": dict(x=x.double(), q=4),
        "numpy x": dict(x=np.zeros((3, 100), np.float32), q=4),
        "strided samples": dict(x=x[:, ::2], q=4),
        "pitch < T": dict(x=torch.as_strided(x, (3, 100), (50, 1)), q=4),
        "out is x": dict(x=x, q=4, out=x[:, :25]),
        "out inside x": dict(x=x, q=4, out=x[:, 60:85]),
        "out overlaps x's end": dict(x=x[:2], q=4, out=torch.as_strided(x, (2, 25), (25, 1), 190)),  # another start address
        "device_taps of another length": dict(x=x, q=4, device_taps=torch.ones(5, dtype=torch.float64)),
        "device_taps float32": dict(x=x, q=4, device_taps=torch.ones(81)),
        "out shape": dict(x=x, q=4, out=torch.zeros((3, 26))),
        "out dtype": dict(x=x, q=4, out=torch.zeros((3, 25), dtype=torch.float64)),
        "out pitch": dict(x=x, q=4, out=torch.as_strided(torch.zeros(100), (3, 25), (20, 1))),
        "host x": dict(x=x, q=4),  # the last refusal: everything else about this call is in order
    }
    for name, kw in bad.items():
        with pytest.raises(ValueError):
            downsample.decimate(**kw)
            pytest.fail(name)


def test_taps_of_a_non_positive_truncated_sum_are_refused():
    x = torch.zeros((2, 64), dtype=torch.float32)
    # the full sum is 1, but the first output keeps only taps H .. 2 H: -1 + 0.5
    h = np.array([1.0, 0.5, -1.0, 0.5, 0.0])
    assert downsample.truncated_sums(h, 64, 2)[0] == pytest.approx(-0.5) and h.sum() == 1.0
    with pytest.raises(ValueError, match="truncated sum"):
        downsample.decimate(x, 2, taps=h)
    with pytest.raises(ValueError, match="truncated sum"):
        downsample.decimate(x, 2, taps=np.array([1.0, 0.0, -1.0]))  # sums to 0 in the interior
    with pytest.raises(ValueError, match="truncated sum"):
        downsample.decimate(x, 2, taps=-downsample.design_taps(2))
    # positive sums everywhere: only the host tensor is left to refuse
    assert np.all(downsample.truncated_sums(downsample.design_taps(2), 64, 2) > 0)
    with pytest.raises(ValueError, match="device tensor"):
        downsample.decimate(x, 2)
