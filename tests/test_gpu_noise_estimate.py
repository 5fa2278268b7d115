"""mrx_tod_welch against scipy.signal.welch, the noise fit on the simulator's known law, and what the fitted weights and
knees are worth to the destriper (maria_amd/noise_estimate.py)."""

import ctypes as C

import numpy as np
import pytest
import scipy.signal
from test_host_noise_estimate import RECOVERY

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = [256, 512, 1024, 2048, 4096, 8192]
# per row: max |got - ref| / max |ref|, and |got - ref| / ref on the bins above BIN_FLOOR of the row's max
ROW_TOL, BIN_TOL, BIN_FLOOR = 2e-6, 1e-4, 1e-6


def _rows(T, fs, n, rng):
    """white, 1/f, a sinusoid on a bin centre (over a little white noise), white on a DC offset of 1e4 rms"""
    from oracle.noise import generate_noise_with_knee

    t = np.arange(T) / fs
    white = rng.normal(size=T)
    pink = generate_noise_with_knee((1, T), sample_rate=fs, knee=10.0, rng=rng)[0]
    sine = 3.0 * np.sin(2 * np.pi * (n // 8) * fs / n * t + 0.3) + 1e-2 * rng.normal(size=T)
    dc = 1e4 + rng.normal(size=T)
    return np.stack([white, pink, sine, dc]).astype(np.float32)


def _welch(ctx, x, T, nperseg, fs, ld=None):
    """mrx_tod_welch of the first T samples of the rows of x (a [D, ld] device tensor)"""
    import torch

    from maria_amd._lib import ptr

    psd = torch.empty((x.shape[0], nperseg // 2 + 1), dtype=torch.float32, device=DEV)
    ctx.call("mrx_tod_welch", ptr(x), x.stride(0) if ld is None else ld, x.shape[0], T, nperseg, fs, ptr(psd))
    torch.cuda.synchronize()
    return psd.cpu().numpy()


def _reference(rows, fs, nperseg):
    """scipy.signal.welch of the float32 rows, evaluated in float64: scipy's own float32 path rounds each segment's mean
    to float32, which on the DC-offset row leaves 1e4 x 6e-8 rms in every segment (2e-4 of the row's max in bin 0); the
    kernel sums the means in float64 and is compared with the exact value"""
    return scipy.signal.welch(rows.astype(np.float64), fs, nperseg=nperseg)[1]


def _check(got, ref, what):
    assert got.shape == ref.shape, what
    for d in range(ref.shape[0]):
        top = np.abs(ref[d]).max()
        err = np.abs(got[d].astype(np.float64) - ref[d])
        assert err.max() <= ROW_TOL * top, (what, d, err.max() / top)
        big = ref[d] > BIN_FLOOR * top
        rel = (err[big] / ref[d][big]).max()
        assert rel <= BIN_TOL, (what, d, rel)


@pytest.mark.parametrize("nperseg", LENGTHS)
def test_welch_matches_scipy(gpu_ctx, nperseg):
    """Every supported length, on T = nperseg (one segment), an odd segment count, T not a multiple of nperseg / 2 (an
    even count, trailing samples dropped) and a long row; rows stored with ld > T, the padding NaN (never read)."""
    import torch

    fs = 37.0
    h = nperseg // 2
    rng = np.random.default_rng(nperseg)
    for T in (nperseg, nperseg + 4 * h, nperseg + 7 * h + 37, 40 * nperseg + 3 * h + 11):
        rows = _rows(T, fs, nperseg, rng)
        ld = T + 67
        buf = np.full((rows.shape[0], ld), np.nan, np.float32)
        buf[:, :T] = rows
        got = _welch(gpu_ctx, torch.as_tensor(buf).to(DEV), T, nperseg, fs)
        _check(got, _reference(rows, fs, nperseg), (nperseg, T))


@pytest.mark.parametrize("nperseg", [256, 4096])
def test_welch_many_rows_and_one(gpu_ctx, nperseg):
    """D = 1 and D = 1031 (a NaN in one row spoils that row only); noise_estimate.welch returns scipy's frequencies."""
    import torch

    from maria_amd import noise_estimate

    fs, T = 100.0, 20_011
    rng = np.random.default_rng(7)
    x = (rng.normal(size=(1031, T)) * rng.uniform(0.5, 3.0, (1031, 1)) + rng.uniform(-50, 50, (1031, 1))).astype(np.float32)
    x[17, 5000] = np.nan
    d_x = torch.as_tensor(x).to(DEV)
    f, psd = noise_estimate.welch(d_x, fs, nperseg=nperseg, ctx=gpu_ctx)
    torch.cuda.synchronize()
    ref_f, ref = scipy.signal.welch(x.astype(np.float64), fs, nperseg=nperseg)
    assert np.array_equal(f.cpu().numpy(), ref_f)
    got = psd.cpu().numpy()
    assert np.isnan(got[17]).all()
    keep = np.arange(1031) != 17
    _check(got[keep], ref[keep], (nperseg, "D 1031"))
    one = _welch(gpu_ctx, d_x[:1].contiguous(), T, nperseg, fs)
    _check(one, ref[:1], (nperseg, "D 1"))
    assert np.array_equal(one, got[:1])


def test_welch_refusals_leave_the_output_untouched(gpu_ctx):
    import torch

    from maria_amd._lib import ptr

    x = torch.zeros((4, 3000), dtype=torch.float32, device=DEV)
    psd = torch.full((4, 513), 7.0, dtype=torch.float32, device=DEV)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    cases = {  # name: (args, status)
        "T < nperseg": ((ptr(x), 3000, 4, 1000, 1024, 50.0, ptr(psd)), -1),
        "ld < T": ((ptr(x), 2999, 4, 3000, 1024, 50.0, ptr(psd)), -1),
        "D < 1": ((ptr(x), 3000, 0, 3000, 1024, 50.0, ptr(psd)), -1),
        "fs 0": ((ptr(x), 3000, 4, 3000, 1024, 0.0, ptr(psd)), -1),
        "null x": ((None, 3000, 4, 3000, 1024, 50.0, ptr(psd)), -1),
        "nperseg 1000": ((ptr(x), 3000, 4, 3000, 1000, 50.0, ptr(psd)), -4),
        "nperseg 128": ((ptr(x), 3000, 4, 3000, 128, 50.0, ptr(psd)), -4),
        "nperseg 16384": ((ptr(x), 3000, 4, 3000, 16384, 50.0, ptr(psd)), -4),
    }
    for name, (args, status) in cases.items():
        assert lib.mrx_tod_welch(h, *args) == status, name
    assert lib.mrx_tod_welch(h, ptr(x), 3000, 4, 3000, 1024, 50.0, None) == -1
    torch.cuda.synchronize()
    assert bool((psd == 7.0).all())


def _two_band_sim(NEP, knee, duration=600.0, sky=True, npos=150):
    """Simulation(noise=True) of a focal plane split into two groups of detectors (alternate positions), two bands at the
    same centre with their own NEP and knee; with `sky` the IQU blob map of test_gpu_destripe's 1/f front end."""
    from maria_amd import map as mmap
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation, sky_transform_stack
    from oracle import mapsample

    bands = [Band(center=150e9, width=40e9, name=f"f150{c}", NEP=nep, knee=k) for c, nep, k in zip("ab", NEP, knee)]
    width = 1.0
    pos = synthetic.hex_pack(npos, np.radians(width / 2))
    group = np.arange(npos) % 2
    gamma = np.radians([0.0, 45.0, 90.0, 135.0])[(np.arange(npos) // 2) % 4]
    dets = Detectors(pos, bands, group, primary_size=1000.0, gamma=gamma)
    plan = Plan.daisy(start_time=1.7e9, duration=duration, sample_rate=50.0, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
    site = Site(altitude=5190.0)
    noise_kwargs = {"correlated_noise_proportion": 0.0, "exact_spectrum": True}
    if not sky:
        sim = Simulation(Instrument(dets), plan, site, noise=True, noise_seed=5, noise_kwargs=noise_kwargs)
        (tod,) = sim.run(units="pW")
        return tod, group
    transform = sky_transform_stack(plan.time, site.latitude, site.longitude)
    phi, theta = mapsample.frame_angles(plan.phi.astype(np.float32)[None], plan.theta.astype(np.float32)[None], transform)
    xyz = mapsample.phi_theta_to_xyz(phi[0], theta[0]).astype(float).mean(axis=0)
    xyz /= np.linalg.norm(xyz)
    centre = (float(np.arctan2(xyz[1], xyz[0]) % (2 * np.pi)), float(np.arcsin(xyz[2])))
    n = 32
    res = width / (n - 1)
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    blob = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0
    data = np.stack([s * blob[None] for s in (1.0, 0.2, -0.1)]).astype(np.float32)
    skymap = mmap.ProjectionMap(data, nu=[150e9], stokes="IQU", width=width, center=np.degrees(centre), frame="ra/dec")
    sim = Simulation(Instrument(dets), plan, site, map=skymap, noise=True, noise_seed=3, noise_kwargs=noise_kwargs)
    (tod,) = sim.run()
    return tod, group, skymap, centre, n, res


def test_fit_recovers_the_simulated_noise_law(gpu_ctx):
    """Noise only, in pW, correlated part off and the exact spectrum: per band the fitted white level is
    2 (1e12 NEP)^2 (oracle.noise.one_sided_psd_model's) and the knee Band.knee, within the host test's bounds for the
    same (fs, knee, T, nperseg)."""
    from oracle.noise import one_sided_psd_model

    bounds = {knee: (wt, kt) for fs, knee, T, n, wt, kt in RECOVERY if fs == 50.0 and T == 30_000}
    NEP, knee = (4e-16, 1.6e-15), (20.0, 0.5)
    tod, group = _two_band_sim(NEP, knee, sky=False, npos=40)
    fit = tod.fit_noise(nperseg=1024, ctx=gpu_ctx)
    for g in (0, 1):
        white = fit["white"].cpu().numpy()[group == g]
        kn = fit["knee"].cpu().numpy()[group == g]
        level = one_sided_psd_model(1e9, 50.0, 0.0, scale=1e12 * NEP[g])
        assert abs(level / (2 * (1e12 * NEP[g]) ** 2) - 1) < 1e-12
        wt, kt = bounds[knee[g]]
        assert abs(white.mean() / level - 1) <= wt, (g, white.mean() / level)
        assert abs(kn.mean() / knee[g] - 1) <= kt, (g, kn.mean() / knee[g])


def _residual_rms(mapper, out, sky):
    """hits-weighted rms of (map - input) over the solved pixels and planes, each plane up to its weighted mean"""
    solved = np.isfinite(out.data[:, 0]).all(axis=0)
    w = mapper.products["weight"][0, 0][solved]
    tot = 0.0
    for s in range(3):
        r = out.data[s, 0][solved].astype(np.float64) - sky.data[s, 0][solved]
        r = r - np.sum(w * r) / np.sum(w)
        tot += np.sum(w * r * r) / np.sum(w)
    return float(np.sqrt(tot / 3))


def test_fitted_noise_pays_on_a_mixed_focal_plane(gpu_ctx, capsys):
    """The destriper's 1/f simulation with two detector groups, white levels 4x apart (NEP 4e-16 and 8e-16) and knees
    10x apart (2 Hz on the quieter group, 20 Hz on the noisier), 0.32 s baselines: the fitted weights and knees
    (noise_weights="fit", baseline_prior={"knee": "fit"}) against the truth (1 / sigma_d^2 from NEP and the K_RJ
    calibration, the bands' knees, alpha 1) and against "inverse_variance" without a prior.  Measured on an MI355X (noise
    seed 3): fitted 9.148e-4 K_RJ, truth 9.175e-4, "inverse_variance" 1.0174e-3 (1.11x the fitted run); the bound is 1.08.
    With the groups' knees the other way round (20 Hz on the quieter group) the fitted run gave 1.498e-3, the truth 1.491e-3
    and "inverse_variance" 1.513e-3: the total variance then misweights the groups less."""
    import torch

    from maria_amd.mappers import DestripingMapper

    NEP, knee = (4e-16, 8e-16), (2.0, 20.0)
    tod, group, sky, centre, n, res = _two_band_sim(NEP, knee)
    # the K_RJ calibration of each detector: the pW TOD of the same simulation, divided into this one
    pw = tod.to("pW")
    k_rj = np.median(np.asarray(tod.signal.cpu() if isinstance(tod.signal, torch.Tensor) else tod.signal, np.float64)
                     / np.asarray(pw.signal.cpu() if isinstance(pw.signal, torch.Tensor) else pw.signal, np.float64), axis=1)
    sigma = 1e12 * np.asarray(NEP)[group] * np.sqrt(50.0) * np.abs(k_rj)
    kw = dict(center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="IQU", nu=[150e9], frame="ra/dec",
              units="K_RJ", tol=1e-8, max_iter=500, baseline_length=0.32)
    runs = {
        "fitted": dict(noise_weights="fit", baseline_prior={"knee": "fit"}),
        "truth": dict(noise_weights=1.0 / sigma**2, baseline_prior={"knee": np.asarray(knee)[group], "alpha": 1.0}),
        "inverse_variance": dict(noise_weights="inverse_variance"),
    }
    r, fits = {}, None
    for name, extra in runs.items():
        mapper = DestripingMapper([tod], **kw, **extra)
        out = mapper.run()
        assert mapper.products["converged"], name
        r[name] = _residual_rms(mapper, out, sky)
        if name == "fitted":
            fits = mapper.products["noise"][0]
    sig_err = [np.median(fits["sigma"][group == g] / sigma[group == g]) for g in (0, 1)]
    knee_fit = [np.median(fits["knee"][group == g]) for g in (0, 1)]
    with capsys.disabled():
        print("\nmixed focal plane, residual rms (K_RJ): " + ", ".join(f"{k} {v:.4e}" for k, v in r.items())
              + f"; fitted sigma / true {sig_err[0]:.4f} {sig_err[1]:.4f}, knees {knee_fit[0]:.3f} {knee_fit[1]:.3f} Hz,"
              f" alpha {np.median(fits['alpha']):.3f}")
    assert all(abs(s - 1) <= 0.05 for s in sig_err), sig_err
    assert r["fitted"] <= 1.05 * r["truth"], r
    assert r["fitted"] * PAYS_BOUND <= r["inverse_variance"], r


PAYS_BOUND = 1.08
