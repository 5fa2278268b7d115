"""Host tier of the band powers: the float64 oracle of tests/bandpower_ref.py against cmb_ref's estimator
and, as an estimator, against the spectra that went in; the host half of maria_amd.bandpowers (edges, taper, the mask of
window_from_weight, the normalisation, nu_b, the beam and transfer divisions, expected) in closed form.  No GPU: the
device's sums are held to this oracle by tests/test_gpu_bandpowers.py."""

import numpy as np
import pytest

import bandpower_ref as ref
import cmb_ref
from maria_amd import bandpowers as bp
from maria_amd import cmb

ARCMIN = np.radians(1.0 / 60.0)
NY, NX, RES = 128, 256, 2 * ARCMIN
EDGES = 100.0 + 200.0 * np.arange(39)  # [100, 7700): past the corner of the plane (7637)


def _realisation(seed, cl):
    table = cmb.spectrum_table(cl, NX * RES, NY * RES)
    g = cmb_ref.numpy_normals(np.random.default_rng(seed), NY, NX)
    return cmb_ref.fields(cmb_ref.half_spectra(g, NY, NX, RES, table), NY, NX), table


def _powers(tqu, tqu2=None, edges=EDGES):
    a1, w = ref.modes(tqu, None, RES)
    a2 = a1 if tqu2 is None else ref.modes(tqu2, None, RES)[0]
    s, _ = ref.sums(a1, a2, RES, edges)
    return bp.from_sums(s, edges, (NY, NX), RES)


def test_oracle_agrees_with_cmb_ref_binned():
    """cmb_ref.binned weighs every independent cell (0 < fx < nx/2) against its own C(l); the oracle fed the same modes
    divided by sqrt C(l), with the column fx = 0 emptied, must give twice binned's sum (w = 2), and its sum w must be
    2 N + the bin's cells of that column: TT and EE to 1e-10 in every bin binned defines."""
    tqu, table = _realisation(3, cmb.toy_spectrum(9000))
    bins = cmb_ref.binned(tqu, RES, table)
    assert len(bins) >= 10
    a = np.fft.rfft2(tqu, axes=(-2, -1)) / (NY * NX)
    ell, _, _ = cmb_ref.rotation(NY, NX, RES)
    area = (NY * RES) * (NX * RES)
    cT, cTE, cE, _ = cmb_ref.coefficients(table, ell) * np.sqrt(area)
    c_tt, c_ee = cT * cT, cTE * cTE + cE * cE
    ok = (c_tt > 0) & (c_ee > 0)
    white = np.zeros_like(a)
    white[0][ok] = a[0][ok] * np.sqrt(area / c_tt[ok])
    white[1][ok] = a[1][ok] * np.sqrt(area / c_ee[ok])
    white[2][ok] = a[2][ok] * np.sqrt(area / c_ee[ok])
    white[:, :, 0] = 0.0
    s, _ = ref.sums(white, white, RES, EDGES)
    _, _, _, _, b = ref.cells(NY, NX, RES, EDGES)
    by_lo = {x["lo"]: x for x in bins}
    seen = 0
    for i, lo in enumerate(EDGES[:-1]):
        if lo not in by_lo:
            continue
        x = by_lo[lo]
        seen += 1
        assert s[i, 0] == 2 * x["N"] + np.count_nonzero(b[:, 0] == i)
        assert abs(s[i, 2] / 2 - x["tt"] * x["N"]) <= 1e-10 * x["tt"] * x["N"], lo
        assert abs(s[i, 3] / 2 - x["ee"] * x["N"]) <= 1e-10 * x["ee"] * x["N"], lo
    assert seen == len(bins)


SEEDS = tuple(range(100, 120))


def test_estimator_statistics_on_twenty_realisations():
    """Whole periodic domain, unit window, C_BB = 0.1 C_EE so that TB and EB have a variance to be held to.  Over 20
    realisations, in every bin with N_b = sum w / 2 >= 400 independent cells: the mean of C_b / expected within
    5 / sqrt(20 N_b) of 1 in TT and EE (and BB), the mean TB and EB within 5 sigma of 0 with the variance of one cell's
    Re(a_X conj a_B) Lx Ly = C_XX C_BB / 2 (cmb_ref.binned's var_te with C_XB = 0), averaged over the bin's cells.
    With C_BB = 0: sum BB / sum EE below 1e-20."""
    cl = cmb.toy_spectrum(9000)
    cl[:, 2] = 0.1 * cl[:, 1]
    got = np.stack([_powers(_realisation(seed, cl)[0]).cl for seed in SEEDS])
    one = _powers(_realisation(SEEDS[0], cl)[0])
    want = ref.expected(cl, NY, NX, RES, EDGES)
    np.testing.assert_array_equal(bp.expected(cl, one), want)
    n_b = one.n_modes / 2
    full = n_b >= 400
    assert full.sum() >= 10
    mean = got.mean(axis=0)
    for col, name in ((0, "TT"), (1, "EE"), (2, "BB")):
        dev = np.abs(mean[full, col] / want[full, col] - 1) * np.sqrt(20 * n_b[full])
        print(f"{name}: largest |mean C_b / expected - 1| sqrt(20 N_b) = {dev.max():.2f}")
        assert dev.max() <= 5, name
    pair_cl = cl.copy()
    pair_cl[:, 0], pair_cl[:, 1] = cl[:, 0] * cl[:, 2] / 2, cl[:, 1] * cl[:, 2] / 2  # the bin means of C_TT C_BB / 2 and C_EE C_BB / 2
    var = ref.expected(pair_cl, NY, NX, RES, EDGES)
    for col, v, name in ((4, var[:, 0], "TB"), (5, var[:, 1], "EB")):
        dev = np.abs(mean[full, col]) / np.sqrt(v[full] / (20 * n_b[full]))
        print(f"{name}: largest |mean| / sigma = {dev.max():.2f}")
        assert dev.max() <= 5, name
    pure_e = _powers(_realisation(SEEDS[0], cmb.toy_spectrum(9000))[0])
    sums_bb = np.nansum(pure_e.cl[:, 2] * pure_e.n_modes)
    sums_ee = np.nansum(pure_e.cl[:, 1] * pure_e.n_modes)
    print(f"BB / EE with C_BB = 0: {sums_bb / sums_ee:.2e}")
    assert 0 <= sums_bb <= 1e-20 * sums_ee


def test_cross_spectrum_carries_no_noise_bias():
    """Two maps share a signal and carry independent white noise of variance s^2 a pixel, N = s^2 res^2 in every
    spectrum.  Against the noiseless signal's own band powers S_b (the realisation's, so no cosmic variance): the auto
    spectrum is high by N within 5 sqrt((2 S_b N + N^2) / N_b), the cross spectrum is not, within
    5 sqrt((S_b N + N^2 / 2) / N_b) -- and N is far outside that, so the test tells the two apart."""
    signal, _ = _realisation(7, cmb.toy_spectrum(9000))
    rng = np.random.default_rng(8)
    s = 20e-6
    m1 = signal + s * rng.standard_normal(signal.shape)
    m2 = signal + s * rng.standard_normal(signal.shape)
    noise = s * s * RES * RES
    clean, auto, cross = _powers(signal), _powers(m1), _powers(m1, m2)
    n_b = clean.n_modes / 2
    full = n_b >= 400
    assert full.sum() >= 10
    for col in (0, 1):
        S = clean.cl[full, col]
        sig_auto = np.sqrt((2 * S * noise + noise**2) / n_b[full])
        sig_cross = np.sqrt((S * noise + noise**2 / 2) / n_b[full])
        assert (np.abs(auto.cl[full, col] - S - noise) <= 5 * sig_auto).all()
        assert (np.abs(cross.cl[full, col] - S) <= 5 * sig_cross).all()
        assert (noise > 10 * sig_cross).all()
    np.testing.assert_array_equal(cross.n_modes, auto.n_modes)


def test_taper_closed_form():
    ny, nx, frac = 40, 64, 0.25
    t = bp.taper(ny, nx, frac)
    assert t.shape == (ny, nx) and t.dtype == np.float64
    np.testing.assert_array_equal(t, t[::-1, ::-1])
    np.testing.assert_allclose(t, np.outer(t[:, nx // 2], t[ny // 2, :]), rtol=1e-15)
    for n, line in ((ny, t[:, nx // 2]), (nx, t[ny // 2, :])):
        m = frac * n / 2
        d = np.arange(n) + 0.5
        hann = np.where(d < m, 0.5 * (1 - np.cos(np.pi * d / m)), 1.0)  # the Hann edge at pixel centres
        np.testing.assert_allclose(line[: n // 2], hann[: n // 2], rtol=1e-13)
        assert np.count_nonzero(line < 1) == 2 * int(np.ceil(m - 0.5))
    assert (bp.taper(8, 8, 0.0) == 1).all()
    assert 0 < bp.taper(16, 16, 1.0).max() < 1  # frac = 1: the two edges meet, no pixel centre sits on the peak
    with pytest.raises(ValueError):
        bp.taper(8, 8, 1.5)


def test_weight_mask_thresholds_at_a_tenth_of_the_median_hit():
    w = np.zeros((6, 8))
    w[1:5, 1:7] = 10.0     # 24 pixels: the median of the positive weights is 10
    w[1, 1] = 0.99         # below 0.1 x 10
    w[1, 2] = 1.01         # above
    w[0, 0] = np.nan       # never hit
    w[5, 7] = -3.0
    m = bp.weight_mask(w)
    want = np.zeros((6, 8))
    want[1:5, 1:7] = 1.0
    want[1, 1] = 0.0
    np.testing.assert_array_equal(m, want)
    assert bp.weight_mask(w, floor=0.05)[1, 1] == 1.0
    with pytest.raises(ValueError):
        bp.weight_mask(np.zeros((4, 4)))


def test_nu_b_is_the_count_of_full_plane_cells_for_a_unit_window():
    """n_modes and nu_b (read back from sigma = C sqrt(2 / nu)) against a count over the full fft2 plane: the cells with
    the bin's l, off both Nyquist lines, k = 0 apart; a window scales nu_b by <W^2>^2 / <W^4>."""
    tqu, _ = _realisation(5, cmb.toy_spectrum(9000))
    edges = np.array([0.0, 150.0, 151.0, 900.0, 2500.0])
    a, _ = ref.modes(tqu, None, RES)
    s, _ = ref.sums(a, a, RES, edges)
    got = bp.from_sums(s, edges, (NY, NX), RES)
    fy = np.fft.fftfreq(NY, 1.0 / NY)[:, None]
    fx = np.fft.fftfreq(NX, 1.0 / NX)[None, :]
    ell = 2 * np.pi * np.hypot(fx / (NX * RES), fy / (NY * RES))
    keep = (np.abs(fy) != NY // 2) & (np.abs(fx) != NX // 2) & (ell > 0)
    count = np.array([np.count_nonzero(keep & (ell >= lo) & (ell < hi)) for lo, hi in zip(edges[:-1], edges[1:])])
    np.testing.assert_array_equal(got.n_modes, count)
    assert count[1] == 0 and np.isnan(got.cl[1]).all() and np.isnan(got.ell[1]) and np.isnan(got.sigma[1]).all()
    live = count > 0
    np.testing.assert_allclose(2 * (got.cl[live, 0] / got.sigma[live, 0]) ** 2, count[live], rtol=1e-12)
    te = np.sqrt((got.cl[live, 0] * got.cl[live, 1] + got.cl[live, 3] ** 2) / count[live])
    np.testing.assert_allclose(got.sigma[live, 3], te, rtol=1e-12)
    W = bp.taper(NY, NX, 0.3)
    tapered = bp.from_sums(s, edges, (NY, NX), RES, w12=np.mean(W**2), w1122=np.mean(W**4))
    np.testing.assert_allclose(tapered.cl[live], got.cl[live] / np.mean(W**2), rtol=1e-14)
    nu = 2 * (tapered.cl[live, 0] / tapered.sigma[live, 0]) ** 2
    np.testing.assert_allclose(nu, count[live] * np.mean(W**2) ** 2 / np.mean(W**4), rtol=1e-12)


def test_beam_and_transfer_divisions_and_dl():
    tqu, _ = _realisation(6, cmb.toy_spectrum(9000))
    edges = bp.bin_edges(100, 400, 3000)
    np.testing.assert_array_equal(edges, 100.0 + 400.0 * np.arange(8))
    a, _ = ref.modes(tqu, None, RES)
    s, _ = ref.sums(a, a, RES, edges)
    plain = bp.from_sums(s, edges, (NY, NX), RES)
    ell_ref, cl_ref, n_ref = ref.band_powers(s, NY, NX, RES, np.ones((NY, NX)))
    np.testing.assert_array_equal(plain.ell, ell_ref)
    np.testing.assert_allclose(plain.cl, cl_ref, rtol=1e-15)
    np.testing.assert_array_equal(plain.n_modes, n_ref)
    fwhm = 5 * ARCMIN
    sigma = fwhm / np.sqrt(8 * np.log(2))
    beamed = bp.from_sums(s, edges, (NY, NX), RES, beam_fwhm=fwhm)
    np.testing.assert_allclose(beamed.cl / plain.cl, np.exp(plain.ell * (plain.ell + 1) * sigma**2)[:, None] * np.ones(6), rtol=1e-13)
    tf1 = np.linspace(0.5, 1.0, 7)
    np.testing.assert_allclose(bp.from_sums(s, edges, (NY, NX), RES, transfer=tf1).cl, plain.cl / tf1[:, None], rtol=1e-15)
    tf6 = np.linspace(0.2, 0.9, 42).reshape(7, 6)
    both = bp.from_sums(s, edges, (NY, NX), RES, beam_fwhm=fwhm, transfer=tf6)
    np.testing.assert_allclose(both.cl, beamed.cl / tf6, rtol=1e-15)
    with pytest.raises(ValueError):
        bp.from_sums(s, edges, (NY, NX), RES, transfer=np.ones(6))
    ell, dl = plain.to_dl()
    np.testing.assert_allclose(dl, plain.cl * (ell * (ell + 1) / (2 * np.pi))[:, None] * 1e12, rtol=1e-15)
    assert plain.columns == ("TT", "EE", "BB", "TE", "TB", "EB") == ref.COLUMNS


def test_edges_are_checked():
    for bad in ([100.0], [100.0, 100.0], [300.0, 200.0], [-1.0, 5.0], [0.0, np.inf], [0.0, np.nan], np.zeros((2, 2)), np.arange(1027.0)):
        with pytest.raises(ValueError):
            bp.check_edges(bad)
    with pytest.raises(ValueError):
        bp.bin_edges(100, 200, 250)
    with pytest.raises(ValueError):
        bp.bin_edges(100, 0, 3000)
    assert bp.bin_edges(0, 50, 125).tolist() == [0.0, 50.0, 100.0]
