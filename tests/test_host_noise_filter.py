"""CPU tier of the inverse-noise filter (maria_amd/noise_filter.py): the lags of the 1/f law are symmetric
by construction, their DTFT is non-negative (the Toeplitz section is positive definite), approaches 2 / (fs P(f)) as K
grows, white noise gives delta / sigma^2 and a failed law gives zero; MaximumLikelihoodMapper's new keywords are checked;
the kernel is bound."""

import ctypes

import numpy as np
import pytest

from maria_amd import _lib, noise_filter


def _dtft(k, omega):
    """sum_t k[|t|] e^{-i omega t} over t = -K..K of the lags k[0..K]"""
    t = np.arange(1, k.size)
    return k[0] + 2.0 * np.cos(np.outer(omega, t)) @ k[1:]


def _inv_psd(f, white, knee, alpha, fs):
    return 2.0 / (fs * white * (1.0 + (knee / f) ** alpha))


@pytest.mark.parametrize("fs", [50.0, 400.0])
@pytest.mark.parametrize("K", [1, 16, 255, 1024, 2048])
def test_lags_have_a_non_negative_dtft(K, fs):
    """every law of a grid of knees and alpha in (0, 2]: DTFT >= 0 down to float64 rounding of the sum"""
    knees = [0.01, 0.5, 2.0, 20.0, fs / 3]
    alphas = [0.3, 1.0, 1.7, 2.0]
    white = 3e-9
    law = [(kn, a) for kn in knees for a in alphas]
    lags = noise_filter.lags(white, [kn for kn, _ in law], [a for _, a in law], fs, K).numpy()
    omega = np.linspace(0.0, np.pi, 8 * K + 4001)
    for (kn, a), k in zip(law, lags):
        H = _dtft(k, omega)
        floor = 1e-12 * np.sum(np.abs(k))
        assert H.min() >= -floor, (K, kn, a, H.min(), floor)


def test_lags_are_symmetric_by_construction_and_match_the_inverse_transform():
    """the lags are k[t] = w_B(t) irfft(2 / (fs P))[t]: the same inverse transform read at -t gives the same value"""
    K, fs, M = 64, 50.0, noise_filter.grid_size(64)
    k = noise_filter.lags(1e-6, 2.0, 1.3, fs, K).numpy()[0]
    f = np.arange(M // 2 + 1) * fs / M
    c = np.zeros(M // 2 + 1)
    c[1:] = _inv_psd(f[1:], 1e-6, 2.0, 1.3, fs)
    full = np.fft.irfft(c, n=M)
    np.testing.assert_allclose(full[1:K + 1], full[::-1][:K], rtol=1e-10, atol=1e-12 * np.abs(full).max())
    bartlett = 1.0 - np.arange(K + 1) / (K + 1)
    np.testing.assert_allclose(k, full[:K + 1] * bartlett, rtol=1e-10, atol=1e-12 * np.abs(full).max())


def test_white_noise_gives_delta_over_sigma_squared():
    white, fs = np.array([1e-6, 4e-12]), 50.0
    k = noise_filter.lags(white, 0.0, np.nan, fs, 300).numpy()
    sigma2 = white * fs / 2
    np.testing.assert_allclose(k[:, 0], 1.0 / sigma2, rtol=1e-15)
    assert np.all(k[:, 1:] == 0.0)


def test_dtft_approaches_the_inverse_spectrum_as_K_grows():
    """knee 2 Hz, alpha 1, fs 50: on f in [10 fs / 128, 0.45 fs] the relative error of the DTFT against 2 / (fs P(f)) shrinks
    with K and is below 0.1 % at K = 2048; above 10 fs / K it stays below 2 % at every K"""
    fs, white, knee, alpha = 50.0, 1e-6, 2.0, 1.0
    errs = []
    for K in (128, 512, 2048):
        k = noise_filter.lags(white, knee, alpha, fs, K).numpy()[0]
        f = np.linspace(10 * fs / 128, 0.45 * fs, 400)
        errs.append(np.max(np.abs(_dtft(k, 2 * np.pi * f / fs) / _inv_psd(f, white, knee, alpha, fs) - 1)))
        f = np.linspace(10 * fs / K, 0.45 * fs, 400)
        assert np.max(np.abs(_dtft(k, 2 * np.pi * f / fs) / _inv_psd(f, white, knee, alpha, fs) - 1)) < 2e-2, K
    assert errs[0] > errs[1] > errs[2], errs
    assert errs[2] < 1e-3, errs


def test_failed_laws_give_zero_lags():
    k = noise_filter.lags([1e-6, np.nan, 1e-6, 1e-6, -1.0, 1e-6], [2.0, 2.0, np.nan, 2.0, 2.0, np.inf], [1.0, 1.0, 1.0, np.nan, 1.0, 1.0],
                          50.0, 100).numpy()
    assert np.all(k[1:] == 0.0)
    assert k[0, 0] > 0


def test_lags_refuse_bad_arguments():
    with pytest.raises(ValueError):
        noise_filter.lags(1.0, 1.0, 1.0, 50.0, 2049)
    with pytest.raises(ValueError):
        noise_filter.lags(1.0, 1.0, 1.0, 50.0, -1)
    with pytest.raises(ValueError):
        noise_filter.lags(1.0, 1.0, 1.0, 0.0, 10)
    with pytest.raises(ValueError):
        noise_filter.lags([1.0, 1.0], [1.0, 1.0, 1.0], 1.0, 50.0, 10)


def test_the_kernel_is_bound():
    restype, argtypes = _lib.SIGNATURES["mrx_tod_noise_filter"]
    v, sz = ctypes.c_void_p, ctypes.c_size_t
    assert restype is ctypes.c_int
    assert argtypes == [v, v, sz, v, sz, ctypes.c_int, ctypes.c_int, v, ctypes.c_int, v, sz]


def _tod(D=8, T=500, fs=50.0):
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t, radius_deg=0.3)
    pos = synthetic.hex_pack(D, np.radians(0.4))
    dets = Detectors(pos, [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int), gamma=np.zeros(D))
    coords = Coordinates(t, az, el, offsets=dets.offsets)
    return TOD({"map": np.zeros((D, T), np.float32)}, dets, coords, units="K_RJ")


def test_mapper_keywords_are_checked():
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod = _tod()
    kw = dict(center=(0.0, 45.0), width=1.0, resolution=0.1, device="cpu")
    MaximumLikelihoodMapper([tod], noise_model="fit", **kw)
    MaximumLikelihoodMapper([tod], noise_model="fit", noise_fit={"nperseg": 256}, **kw)
    MaximumLikelihoodMapper([tod], noise_model={"white": 1.0, "knee": 0.0}, noise_filter_length=2.0, **kw)
    MaximumLikelihoodMapper([tod], noise_model={"white": np.ones(8), "knee": np.full(8, 2.0), "alpha": 1.0}, **kw)
    bad = [
        dict(noise_model="white"),
        dict(noise_model=3.0),
        dict(noise_model={"white": 1.0}),
        dict(noise_model={"white": 1.0, "knee": 1.0}),                      # alpha needed for a knee
        dict(noise_model={"white": 1.0, "knee": 0.0, "sigma": 1.0}),
        dict(noise_model={"white": np.ones(7), "knee": 0.0}),               # one value per detector
        dict(noise_model="fit", noise_weights="uniform"),                    # N^-1 carries the weight
        dict(noise_model="fit", noise_weights="fit"),
        dict(noise_model="fit", noise_weights=np.ones(8)),
        dict(noise_model="fit", noise_filter_length=41.0),                   # 2050 samples
        dict(noise_model="fit", noise_filter_length=-1.0),
        dict(noise_model="fit", noise_filter_length=np.nan),
        dict(noise_filter_length=1.0),                                       # without a model
        dict(noise_model={"white": 1.0, "knee": 0.0}, noise_fit={"nperseg": 256}),  # noise_fit unused
    ]
    for extra in bad:
        with pytest.raises(ValueError):
            MaximumLikelihoodMapper([tod], **kw, **extra)
    with pytest.raises(ValueError):
        MaximumLikelihoodMapper([tod], noise_weights="white", **kw)
