"""CPU tier of the noise estimate (maria_amd/noise_estimate.py): the fit of the noise law on exact model spectra and on
scipy Welch spectra of the oracle's noise, and the argument checks of welch, fit_noise and the mappers' new values."""

import numpy as np
import pytest
import scipy.signal

from maria_amd import noise_estimate
from oracle.noise import generate_noise_with_knee


def _model(f, white, knee, alpha):
    with np.errstate(divide="ignore", over="ignore"):
        return white * (1.0 + (knee / f) ** alpha)


def test_fit_recovers_exact_model_spectra():
    """A grid of (white, knee, alpha), alpha = 2 included, and a white-only row: every parameter to 1e-6 relative."""
    fs, n = 50.0, 1024
    f = np.arange(n // 2 + 1) * fs / n
    grid = [(w, k, a) for w in (1e-3, 2.0, 7e4) for k in (0.2, 1.0, 5.0, 20.0) for a in (0.3, 1.0, 1.5, 2.0)]
    rows = [_model(f, *g) for g in grid] + [np.full(f.size, 3.0)]
    P = np.array(rows)
    P[:, 0] = 0.0  # (the DC bin is outside the default range)
    fit = noise_estimate.fit_noise(f, P)
    for i, (w, k, a) in enumerate(grid):
        got = (float(fit["white"][i]), float(fit["knee"][i]), float(fit["alpha"][i]))
        assert np.allclose(got, (w, k, a), rtol=1e-6, atol=0), ((w, k, a), got)
        assert not bool(fit["knee_at_floor"][i])
    assert abs(float(fit["white"][-1]) / 3.0 - 1) <= 1e-6
    assert bool(fit["knee_at_floor"][-1]) and float(fit["knee"][-1]) <= noise_estimate.KNEE_FLOOR * f[1] * (1 + 1e-9)
    assert np.allclose(fit["sigma"].numpy(), np.sqrt(fit["white"].numpy() * fs / 2))


def test_fit_batches_rows_and_marks_bad_ones():
    fs, n = 100.0, 2048
    f = np.arange(n // 2 + 1) * fs / n
    P = np.array([_model(f, 1.0, 2.0, 1.0), _model(f, 1.0, 2.0, 1.0), _model(f, 4.0, 0.5, 1.7)])
    P[1, 40] = np.nan
    P[:, 0] = 0.0
    fit = noise_estimate.fit_noise(f, P)
    assert np.isnan(float(fit["white"][1])) and np.isnan(float(fit["sigma"][1])) and np.isnan(float(fit["knee"][1]))
    assert abs(float(fit["knee"][2]) / 0.5 - 1) <= 1e-6 and abs(float(fit["white"][0]) - 1) <= 1e-6


# (fs, knee, T, nperseg): mean |error| bounds of white and knee over 20 rows.  A scipy + least_squares prototype gave
# 3 % / 6 %, 0.1 % / 2 %, 1.3 % / 3 %; this fit gave 1.1 % / 2.4 %, 0.23 % / 1.3 %, 1.0 % / 1.2 % (seed 1).  Bounds with
# margin over both.
RECOVERY = [(50.0, 20.0, 30_000, 1024, 0.05, 0.10), (400.0, 1.0, 240_000, 4096, 0.006, 0.04), (50.0, 0.5, 30_000, 1024, 0.03, 0.08)]


@pytest.mark.parametrize("fs,knee,T,nperseg,white_tol,knee_tol", RECOVERY)
def test_fit_recovers_the_oracle_noise(fs, knee, T, nperseg, white_tol, knee_tol):
    """generate_noise_with_knee (unit scale: one-sided white level 2, alpha 1) through scipy.signal.welch and fit_noise."""
    x = generate_noise_with_knee((20, T), sample_rate=fs, knee=knee, rng=np.random.default_rng(1)).astype(np.float32)
    f, p = scipy.signal.welch(x, fs, nperseg=nperseg)
    fit = noise_estimate.fit_noise(f, p)
    assert abs(fit["white"].numpy().mean() / 2.0 - 1) <= white_tol
    assert abs(fit["knee"].numpy().mean() / knee - 1) <= knee_tol
    assert abs(np.median(fit["alpha"].numpy()) - 1) <= 0.1
    assert np.allclose(fit["sigma"].numpy(), np.sqrt(fs), rtol=3 * white_tol)


def test_fit_range_errors():
    f = np.arange(513) * 50.0 / 1024
    P = np.ones((1, 513))
    with pytest.raises(ValueError, match="empty fit range"):
        noise_estimate.fit_noise(f, P, f_min=10.0, f_max=5.0)
    with pytest.raises(ValueError, match="empty fit range"):
        noise_estimate.fit_noise(f, P, f_min=10.0, f_max=10.05)
    with pytest.raises(ValueError, match="n_bins"):
        noise_estimate.fit_noise(f, P, n_bins=2)


def test_welch_argument_errors():
    import torch

    x = torch.zeros((2, 4096))
    for bad in (100, 300, 128, 16384, 2.5, True):
        with pytest.raises(ValueError, match="nperseg .*: a power of two in 256 .. 8192"):
            noise_estimate.welch(x, 50.0, nperseg=bad)
    with pytest.raises(ValueError, match="longer than the row"):
        noise_estimate.welch(x, 50.0, nperseg=8192)
    with pytest.raises(ValueError, match="fs"):
        noise_estimate.welch(x, 0.0, nperseg=256)
    with pytest.raises(ValueError, match="on the GPU"):
        noise_estimate.welch(x, 50.0, nperseg=256)  # a CPU tensor: no CPU fall-back
    assert noise_estimate.default_nperseg(240_000) == 8192 and noise_estimate.default_nperseg(30_000) == 2048
    assert noise_estimate.default_nperseg(1000) == 256


def _tod(n=4, T=2000):
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD

    band = Band(center=150e9, width=40e9, name="f150", NEP=4e-16, knee=1.0)
    dets = Detectors(np.zeros((n, 2)), [band], np.zeros(n, int), primary_size=1000.0, gamma=np.zeros(n))

    class Coords:
        t = np.arange(T) / 50.0

    return TOD({"noise": np.zeros((n, T), np.float32)}, dets, Coords(), units="K_RJ")


def test_mapper_noise_options_are_checked():
    from maria_amd.mappers import DestripingMapper, MaximumLikelihoodMapper

    kw = dict(center=(0, 0), width=1.0, resolution=0.1)
    tods = [_tod()]
    with pytest.raises(ValueError, match="noise_weights 'whitish': 'inverse_variance', 'uniform', 'fit'"):
        MaximumLikelihoodMapper(tods, noise_weights="whitish", **kw)
    with pytest.raises(ValueError, match="noise_fit is used only by"):
        MaximumLikelihoodMapper(tods, noise_fit={"nperseg": 1024}, **kw)
    with pytest.raises(ValueError, match="noise_fit .*: a dict of"):
        MaximumLikelihoodMapper(tods, noise_weights="fit", noise_fit={"segment": 1024}, **kw)
    with pytest.raises(ValueError, match="nperseg 1000"):
        MaximumLikelihoodMapper(tods, noise_weights="fit", noise_fit={"nperseg": 1000}, **kw)
    with pytest.raises(ValueError, match="baseline_prior knee 'guess'"):
        DestripingMapper(tods, baseline_prior={"knee": "guess"}, **kw)
    with pytest.raises(ValueError, match="alpha 'fit' needs knee 'fit'"):
        DestripingMapper(tods, baseline_prior={"knee": 1.0, "alpha": "fit"}, **kw)
    with pytest.raises(ValueError, match="baseline_prior alpha 'steep'"):
        DestripingMapper(tods, baseline_prior={"knee": "fit", "alpha": "steep"}, **kw)
    with pytest.raises(ValueError, match="noise_fit is used only by"):
        DestripingMapper(tods, baseline_prior={"knee": 1.0}, noise_fit={"n_bins": 16}, **kw)
    # accepted: the fit feeds the prior alone, or the weights alone, or both
    m = DestripingMapper(tods, baseline_prior={"knee": "fit"}, noise_fit={"n_bins": 16}, **kw)
    assert m.baseline_prior == {"knee": "fit", "alpha": "fit", "band": 16}
    assert DestripingMapper(tods, baseline_prior={"knee": "fit", "alpha": 1.5}, **kw).baseline_prior["alpha"] == 1.5
    assert MaximumLikelihoodMapper(tods, noise_weights="fit", **kw).noise_weights == "fit"
