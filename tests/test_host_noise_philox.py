"""CPU tier: oracle/noise_philox.py, the float64 rebuild of mrx_noise_generate that tests/test_gpu_noise_philox.py
compares the kernels with draw for draw.  Its Philox is the library's; it follows the documented law (spectrum,
zero pink mean over the TOD, independent rows of a pair, the modes' covariance); and each mistake the GPU test
is there to catch moves its output by far more than that test's bound."""

import ctypes as C

import numpy as np
import pytest

from maria_amd import _lib
from oracle import noise_philox as onp

from test_abi import KAT, _philox_py


def _period(T):
    n1, n2 = C.c_int(), C.c_int()
    assert _lib.load().mrx_noise_period(T, C.byref(n1), C.byref(n2)) == 0
    return n1.value, n2.value


def test_philox_matches_the_known_answers_and_the_library():
    for counter, key, expected in KAT:
        seed = key[0] | (key[1] << 32)
        assert tuple(int(w) for w in onp.philox4x32(*counter, seed)) == expected
    rng = np.random.default_rng(4)
    c = rng.integers(0, 2**32, size=(4, 64), dtype=np.uint64)
    seed = int(rng.integers(0, 2**63)) * 2 + 1
    words = onp.philox4x32(*c, seed)
    for i in range(c.shape[1]):
        counter = tuple(int(v) for v in c[:, i])
        want = tuple(int(w[i]) for w in words)
        assert _philox_py(counter, (seed & 0xFFFFFFFF, seed >> 32)) == want
        assert _lib.philox4x32(seed, counter) == want


def test_box_muller_and_window_factor():
    """Box-Muller of the extreme words; W_k / T in closed form against the direct sum."""
    g = onp.box_muller(np.array([0, 0xFFFFFFFF], np.uint64), np.array([0, 0x40000000], np.uint64))
    assert np.isclose(g[0], np.sqrt(-2 * np.log(0.5 / 2**24)))  # u2 = 0: cos 1, sin 0
    assert abs(g[1].real) < 1e-15 * abs(g[1]) and np.isclose(g[1].imag, np.sqrt(-2 * np.log(1 - 0.5 / 2**24)))  # u2 = 1/4
    n, T = 4096, 2999
    k = np.array([1, 2, 3, 77, 128, 2047, 4095])
    direct = np.exp(2j * np.pi * np.outer(k, np.arange(T)) / n).sum(axis=1) / T
    np.testing.assert_allclose(onp.window_mean_factor(k, n, T), direct, rtol=0, atol=1e-12)


def test_spectrum_follows_the_documented_law():
    """Mean one-sided density of the full period, 512 pairs: 2 (1 + knee / f) from k_min = ceil(N / T) on, the white
    level 2 alone below it; each octave within 4 sampling sigmas.  The periodogram of a whole period is unbiased."""
    T, fs, knee, D = 2900, 50.0, 2.0, 1024
    n1, n2 = _period(T)
    n = n1 * n2
    k_min, _ = onp.window(n, T)
    assert (n, k_min) == (4096, 2)
    x = onp.one_rate(3, D, T, fs, knee, n1, n2, keep=n)
    p = (np.abs(np.fft.rfft(x, axis=1)) ** 2).mean(axis=0) * 2.0 / (fs * n)
    f = np.fft.rfftfreq(n, 1 / fs)
    want = 2.0 * (1.0 + np.where(np.arange(len(f)) >= k_min, knee / np.maximum(f, 1e-30), 0.0))
    assert abs(p[1] / want[1] - 1) < 4 / np.sqrt(D) and want[1] == 2.0  # below fs / T: white only
    lo = k_min
    while lo < n // 2:
        hi = min(2 * lo, n // 2)
        ratio = p[lo:hi].sum() / want[lo:hi].sum()
        assert abs(ratio - 1) < 4 / np.sqrt(D * (hi - lo)), (lo, hi, ratio)
        lo = hi


def test_pink_mean_over_the_tod_is_the_truncation_only():
    """The pink part's mean over the T samples is what the cells from k_cut on carry (the window mean of the cells
    below is subtracted): its variance matches that truncation's, sum_{|k| >= k_cut} (knee / |k|) |W_k / T|^2,
    within sampling error -- and is far below the mean left without the subtraction."""
    T, fs, knee, D = 3001, 50.0, 2.0, 2048
    n1, n2 = _period(T)
    n = n1 * n2
    k_min, k_cut = onp.window(n, T)
    x = onp.one_rate(5, D, T, fs, knee, n1, n2, white=False)
    k = np.arange(1, n)
    kk = np.minimum(k, n - k)
    far = kk >= k_cut
    trunc = np.sum(knee / kk[far] * np.abs(onp.window_mean_factor(k[far], n, T)) ** 2)
    got = np.mean(x.mean(axis=1) ** 2)
    assert abs(got / trunc - 1) < 5 * np.sqrt(2 / D), (got, trunc)
    raw = onp.one_rate(5, D, T, fs, knee, n1, n2, white=False, perturb=("no_window_mean",))
    assert np.mean(raw.mean(axis=1) ** 2) > 1000 * trunc
    # the truncation is what the header promises: a small part of the pink part's own spread
    assert np.sqrt(trunc) < 2e-3 * x.std()


def test_rows_of_a_pair_are_independent_and_modes_follow_the_basis():
    """Re and Im of a pair's series are uncorrelated; with modes the covariance between rows is
    c B B^T var(M) + var(own) I, var(M) = fs + knee sum 1/|k|, var(own) = fs + (1 - c) knee sum 1/|k|."""
    T, fs, knee, c = 65536, 100.0, 0.5, 0.6
    n1, n2 = _period(T)
    n = n1 * n2
    x = onp.one_rate(9, 256, T, fs, knee, n1, n2)
    ab = (x[0::2] * x[1::2]).mean(axis=1) / x.var()
    assert abs(ab.mean()) < 4 * ab.std() / np.sqrt(len(ab))
    D, m = 16, 5
    B = np.random.default_rng(2).normal(size=(D, m)) / np.sqrt(m)
    x = onp.one_rate(9, D, T, fs, knee, n1, n2, corr=c, basis=B)
    kk = np.minimum(np.arange(1, n), n - np.arange(1, n))
    s = np.sum(1.0 / kk)
    model = c * (B @ B.T) * (fs + knee * s) + (fs + (1 - c) * knee * s) * np.eye(D)
    cov = np.cov(x)  # (five realised modes: their sample covariance is off by a few per cent)
    assert np.abs(cov - model).max() < 0.05 * np.diag(model).mean(), np.abs(cov - model).max() / np.diag(model).mean()
    off = ~np.eye(D, dtype=bool)
    assert np.corrcoef(cov[off], model[off])[0, 1] > 0.97


def test_two_rate_form_law():
    """The two-rate form: unit white level at the top of the band (own + modes through the basis), the slow pink
    part below, nothing of it at the top."""
    T, fs, knee, D, c = 65536, 400.0, 1.0, 64, 0.5
    B = np.random.default_rng(3).normal(size=(D, 3)) / np.sqrt(3)
    n1, n2 = _period(-(-T // 4) + 4)
    x = onp.two_rate(11, D, T, fs, knee, 4, n1, n2, corr=c, basis=B)
    p = (np.abs(np.fft.rfft(x, axis=1)) ** 2) * 2.0 / (fs * T)
    f = np.fft.rfftfreq(T, 1 / fs)
    top = p[:, f > 0.4 * fs].mean(axis=1) / (2 * (1 + c * (B**2).sum(axis=1)))
    assert abs(top.mean() - 1) < 0.02
    low = (f > 0.1) & (f < 1.0)
    assert p[:, low].mean() > 3 * top.mean() * 2


# ---- sensitivity: every mistake the GPU test exists for moves the output by far more than its bound -----------


def _worst(ref, bad):
    return float(onp.row_ratios(bad, ref).max())


ONE_RATE = dict(seed=7, D=4, T=2999, fs=50.0, knee=2.0, corr=0.4, det_offset=2)  # N = 4096, k_min = 2


@pytest.mark.parametrize("perturb", ["mode_upper_sign", "no_window_mean", "k_min_minus_1", "swap_cos_sin"])
def test_each_mistake_exceeds_the_bound(perturb):
    n1, n2 = _period(ONE_RATE["T"])
    basis = np.random.default_rng(1).normal(size=(ONE_RATE["D"], 3)) / np.sqrt(3)
    ref = onp.one_rate(n1=n1, n2=n2, basis=basis, **ONE_RATE)
    bad = onp.one_rate(n1=n1, n2=n2, basis=basis, perturb=(perturb,), **ONE_RATE)
    assert _worst(ref, bad) > 30 * onp.GPU_BOUND, _worst(ref, bad)


@pytest.mark.parametrize("T", [3001, 50001, 200001])
def test_one_wrong_cell_above_k_cut_exceeds_the_bound(T):
    """One cell out of N (up to 2^18) changed: every sample moves by ~|X_k|, ~1/sqrt(N) of the row's rms (a cell
    near N / 2, where the white part dominates and the change is smallest: 2.3e-3 of the rms at 2^18)."""
    n1, n2 = _period(T)
    assert n1 * n2 <= 1 << 18
    ref = onp.one_rate(7, 2, T, 50.0, 2.0, n1, n2)
    bad = onp.one_rate(7, 2, T, 50.0, 2.0, n1, n2, perturb=("cell",))
    assert _worst(ref, bad) > 10 * onp.GPU_BOUND, _worst(ref, bad)


@pytest.mark.parametrize("rate,knee", [(4, 1.0), (2, 2.0)])
def test_wrong_catmull_rom_phase_exceeds_the_bound(rate, knee):
    T = 40001
    n1, n2 = _period(-(-T // rate) + 4)
    ref = onp.two_rate(7, 2, T, 400.0, knee, rate, n1, n2)
    bad = onp.two_rate(7, 2, T, 400.0, knee, rate, n1, n2, perturb=("cr_phase",))
    assert _worst(ref, bad) > 30 * onp.GPU_BOUND, _worst(ref, bad)


def test_generate_picks_the_library_forms():
    """two_rate_factor as the library's: rate 4 / 2 at 400 Hz with knees of 1 / 2 Hz from 32 768 samples on."""
    assert onp.two_rate_factor(32768, 400.0, 1.0) == 4 and onp.two_rate_factor(32767, 400.0, 1.0) == 1
    assert onp.two_rate_factor(40001, 400.0, 2.0) == 2 and onp.two_rate_factor(40001, 50.0, 2.0) == 1
    assert onp.two_rate_factor(40001, 400.0, 1.0, one_rate_only=True) == 1
