"""The beam fit on the device (mrx_tod_source_flag, mrx_tod_beam_normal, maria_amd/beamfit.py, TOD.fit_beams)
against its float64 restatement, tests/beamfit_ref.py.

Both kernels launch a plain grid, one workgroup per (tile or chunk of 16 tiles, group of 16 rows): no workgroup strides
over work items, so there is no resident-grid case here.  Off the field centre, at the seams of the tile, the row group
and the chunk, and the C entries' refusals: tests/test_gpu_beamfit_edges.py.

The kernel's pointing is float32 and the reference's float64, so the sums are compared under an envelope and not a
constant: four times the change of the reference's own sum when its offsets move by one float32 spacing, plus float64
summation rounding (beamfit_ref.envelope; the spacing is that of the float32 numbers of magnitude up to 1 the offsets are
formed from, 2^-23 rad: beamfit_ref.SPACING)."""

import numpy as np
import pytest
from test_gpu_jumps import device_rows, untouched_outside

import beamfit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0
CASES = {}


def case_of(frame, drift, K):
    """The shared cases, made once and never changed."""
    key = (frame, drift, K)
    if key not in CASES:
        CASES[key] = R.make_case(frame, drift=drift, K=K)
    return CASES[key]


def pointing_of(case, with_offsets=True):
    import torch

    p = dict(az=torch.as_tensor(case["az"]).to(DEV), el=torch.as_tensor(case["el"]).to(DEV),
             transform=None if case["transform"] is None else torch.as_tensor(np.ascontiguousarray(case["transform"].reshape(-1, 9))).to(DEV))
    if with_offsets:
        p["dx"] = torch.as_tensor(case["nominal"][:, 0].astype(np.float32)).to(DEV)
        p["dy"] = torch.as_tensor(case["nominal"][:, 1].astype(np.float32)).to(DEV)
    return p


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("frame,drift", [("az/el", False), ("ra/dec", True), ("az/el", True), ("ra/dec", False)])
def test_source_flag_against_reference_distances(gpu_ctx, frame, drift, layout):
    """flags |= value inside (and, once more, outside) the radius: equal to the reference's verdict except where the
    reference distance lies within MARGIN float32 spacings of the radius, which (checked first, on the host) is fewer than
    1 % of the samples; earlier bits stay, and nothing outside D x T is written."""
    import torch

    from maria_amd import beamfit

    case = case_of(frame, drift, 5)
    D, T = case["D"], case["T"]
    dist = np.sqrt(case["dist2"])
    rng = np.random.default_rng(5)
    before = rng.choice(np.array([0, 2, 8, 10], np.uint8), size=(D, T))
    src = None if case["src"] is None else torch.as_tensor(case["src"]).to(DEV)
    for radius, inside, value in ((R.RADIUS, True, 1), (0.4 * R.RADIUS, False, 5), (0.0, True, 1)):
        unsure = np.abs(dist - radius) <= MARGIN * R.SPACING
        assert unsure.mean() < 0.01
        hit = dist <= radius if inside else dist > radius
        if radius > 0:
            assert 0.02 < hit.mean() < 0.98  # the radius does cut the scan
        want = np.where(hit, before | np.uint8(value), before)
        buf, view, _ = device_rows(before, layout, 64)
        out = beamfit.source_flags(pointing_of(case), case["center"], radius, src=src, inside=inside, value=value, flags=view, ctx=gpu_ctx)
        torch.cuda.synchronize()
        got = view.cpu().numpy()
        assert out is view
        wrong = (got != want) & ~unsure
        print(f"{frame} drift {drift} {layout} radius {radius:.3e}: {int(unsure.sum())} samples within the spacing, {int((got != want).sum())} differ")
        assert not wrong.any()
        assert np.all((got == before) | (got == (before | np.uint8(value))))
        assert untouched_outside(buf, view, 64)
    new = beamfit.source_flags(pointing_of(case), case["center"], R.RADIUS, src=src, ctx=gpu_ctx).cpu().numpy()
    unsure = np.abs(dist - R.RADIUS) <= MARGIN * R.SPACING
    assert new.dtype == np.uint8 and np.all((new == (dist <= R.RADIUS)) | unsure)


def run_normal(gpu_ctx, case, params, flags, model, layout, fill=7.0):
    """The entry on padded buffers: (Normal as numpy, the buffers and views for the 'unchanged' checks)."""
    import torch

    from maria_amd import beamfit

    xbuf, xv, _ = device_rows(case["x"] if model is None else (case["x"] + model).astype(np.float32), layout, fill)
    fbuf, fv, _ = device_rows(flags, layout, 3)
    mv = mbuf = None
    if model is not None:
        mbuf, mv, _ = device_rows(model, layout, -fill)
    src = None if case["src"] is None else torch.as_tensor(case["src"]).to(DEV)
    par = torch.as_tensor(params).to(DEV)
    keep = [b.clone() for b in (xbuf, fbuf, par) + (() if mbuf is None else (mbuf,))]
    n = beamfit.normal_equations(xv, pointing_of(case, with_offsets=False), case["center"], par, flags=fv, model=mv, src=src, ctx=gpu_ctx)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(keep, (xbuf, fbuf, par) + (() if mbuf is None else (mbuf,))))
    return n, same, (xv, fv, mv, src, par)


@pytest.mark.parametrize("frame,drift,K,with_model,layout", [
    ("az/el", False, 5, False, "aligned"), ("ra/dec", True, 5, True, "odd"), ("ra/dec", False, 7, True, "aligned"),
    ("az/el", True, 7, False, "odd"), ("ra/dec", True, 7, False, "aligned"), ("az/el", False, 5, True, "odd")])
def test_beam_normal_against_reference(gpu_ctx, frame, drift, K, with_model, layout):
    """hits exactly; chi2, JtJ and Jtr within MARGIN envelopes of the reference (the measured ratio is printed: DESIGN
    3.29 records it); a second call and a call with NaN under every flagged sample give the same bits; a row with every
    sample flagged (row 3, and the last row, which never nears the source) gives zeros; inputs unchanged."""
    import torch

    from maria_amd import beamfit

    case = case_of(frame, drift, K)
    flags = R.window_of(case)
    flags[3] = 1
    flags[5, ::7] = 4  # other bits count as flagged too
    params = R.start_of(case)
    model = case["model"] if with_model else None
    x_ref = case["x"] if model is None else (case["x"] + model).astype(np.float32)
    hits, chi2, JtJ, Jtr = R.sums(x_ref, case["G"], params, flags, model, case["src"])
    env = R.envelope(x_ref, case["G"], params, flags, model, case["src"])
    n, same, (xv, fv, mv, src, par) = run_normal(gpu_ctx, case, params, flags, model, layout)
    assert same, "an input changed"
    assert np.array_equal(n.hits.cpu().numpy(), hits) and hits[3] == 0 and hits[-1] == 0 and hits[0] > 100
    got = (n.chi2.cpu().numpy(), n.JtJ.cpu().numpy(), n.Jtr.cpu().numpy())
    assert np.array_equal(got[1], np.swapaxes(got[1], 1, 2))
    for name, g, want, e in zip(("chi2", "JtJ", "Jtr"), got, (chi2, JtJ, Jtr), env):
        assert np.all(g[3] == 0) and np.all(g[-1] == 0), name
        live = hits > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(e[live] > 0, np.abs(g[live] - want[live]) / e[live], np.where(g[live] == want[live], 0.0, np.inf))
        print(f"{frame} drift {drift} K {K} model {with_model} {layout}: {name} largest |kernel - reference| / envelope {ratio.max():.3e}")
        assert ratio.max() <= MARGIN, (name, float(ratio.max()))
    again = beamfit.normal_equations(xv, pointing_of(case, with_offsets=False), case["center"], par, flags=fv, model=mv, src=src, ctx=gpu_ctx)
    assert all(torch.equal(a, b) for a, b in zip(n, again)), "a second call gave other bits"
    xv[fv != 0] = float("nan")
    if mv is not None:
        mv[fv != 0] = float("nan")
    poisoned = beamfit.normal_equations(xv, pointing_of(case, with_offsets=False), case["center"], par, flags=fv, model=mv, src=src, ctx=gpu_ctx)
    assert all(torch.equal(a, b) for a, b in zip(n, poisoned)), "a NaN under a flag changed a bit"
    # without flags every sample counts
    free = beamfit.normal_equations(torch.as_tensor(x_ref).to(DEV), pointing_of(case, with_offsets=False), case["center"], par,
                                    model=None if model is None else torch.as_tensor(model).to(DEV), src=src, ctx=gpu_ctx)
    h0, c0, _, _ = R.sums(x_ref, case["G"], params, None, model, case["src"])
    e0 = R.envelope(x_ref, case["G"], params, None, model, case["src"])[0]
    assert np.array_equal(free.hits.cpu().numpy(), h0) and np.all(np.abs(free.chi2.cpu().numpy() - c0) <= MARGIN * e0)


def test_beam_normal_over_several_chunks(gpu_ctx):
    """T = 16 tiles + 1 tile + 5 samples: two chunks of partial sums per row, the second one short; three rows."""
    case = R.make_case("ra/dec", drift=True, K=7, D=3, T=17 * 1024 + 5)
    flags = R.window_of(case)
    flags[:, 16 * 1024 - 40:16 * 1024 + 40] = 0  # kept samples on both sides of the chunks' seam
    params = R.start_of(case)
    hits, chi2, JtJ, Jtr = R.sums(case["x"], case["G"], params, flags, None, case["src"])
    env = R.envelope(case["x"], case["G"], params, flags, None, case["src"])
    n, same, _ = run_normal(gpu_ctx, case, params, flags, None, "odd")
    assert same and np.array_equal(n.hits.cpu().numpy(), hits) and hits[:2].min() > 1000
    for name, g, want, e in zip(("chi2", "JtJ", "Jtr"), (n.chi2, n.JtJ, n.Jtr), (chi2, JtJ, Jtr), env):
        live = hits > 0
        diff = np.abs(g.cpu().numpy()[live] - want[live])
        ratio = np.where(e[live] > 0, diff / np.where(e[live] > 0, e[live], 1.0), np.where(diff == 0, 0.0, np.inf))
        print(f"two chunks: {name} largest |kernel - reference| / envelope {ratio.max():.3e}")
        assert ratio.max() <= MARGIN


def test_chain_option_is_unsupported(gpu_ctx):
    import torch

    from maria_amd import beamfit
    from maria_amd._lib import MrxError

    case = case_of("az/el", False, 5)
    flags = torch.zeros((case["D"], case["T"]), dtype=torch.uint8, device=DEV)
    x = torch.as_tensor(case["x"]).to(DEV)
    gpu_ctx.set_option(0, 1)
    try:
        with pytest.raises(MrxError) as e:
            beamfit.source_flags(pointing_of(case), case["center"], R.RADIUS, flags=flags, ctx=gpu_ctx)
        assert e.value.code == -4
        with pytest.raises(MrxError) as e:
            beamfit.normal_equations(x, pointing_of(case), case["center"], torch.as_tensor(R.start_of(case)).to(DEV), flags=flags, ctx=gpu_ctx)
        assert e.value.code == -4
    finally:
        gpu_ctx.set_option(0, 0)
    torch.cuda.synchronize()
    assert not bool(flags.any()), "the refused call wrote flags"


@pytest.mark.parametrize("frame,drift,K", [("ra/dec", True, 5), ("az/el", False, 7)])
def test_fit_on_injected_truth(gpu_ctx, frame, drift, K):
    """Noiseless: the device fit agrees with the numpy Levenberg-Marquardt of the reference on the same data within the
    envelope of Jtr at the optimum carried through (JtJ)^-1, plus ten times the stopping tolerance of the two
    iterations.  White noise of known sigma: |fit - truth| < 5 reported sigmas for every parameter of every detector
    (seed fixed; the reference fit is held to the same first, on the host).  The detector that never crosses the source
    comes back not ok, with NaNs, and the others are what they are without it."""
    import torch

    from maria_amd import beamfit

    case = case_of(frame, drift, K)
    D = case["D"]
    win = R.window_of(case)
    start = R.start_of(case)
    src = None if case["src"] is None else torch.as_tensor(case["src"]).to(DEV)
    tol = 1e-8

    def device_fit(x, rows=slice(None)):
        sub = dict(pointing_of(case))
        sub["dx"], sub["dy"] = sub["dx"][rows].contiguous(), sub["dy"][rows].contiguous()
        return beamfit.fit(torch.as_tensor(x[rows]).to(DEV), sub, case["center"], torch.as_tensor(start[rows]).to(DEV),
                           torch.as_tensor(win[rows]).to(DEV), src=src, elliptical=(K == 7), n_iter=30, tol=tol, ctx=gpu_ctx)

    ref = R.lm_fit(lambda p: R.sums(case["x"], case["G"], p, win, None, case["src"]), start, n_iter=30, tol=tol)
    fit = device_fit(case["x"])
    ok = fit.ok.cpu().numpy()
    assert np.array_equal(ok, ref["ok"]) and ok[:-1].all() and not ok[-1]
    got = fit.params.cpu().numpy()
    assert np.isnan(got[-1]).all() and np.isnan(fit.cov.cpu().numpy()[-1]).all() and np.isnan(float(fit.fwhm[-1])) and np.isnan(float(fit.sigma_dx[-1]))
    _, _, N, _ = R.sums(case["x"][:-1], case["G"], ref["params"][:-1], win[:-1], None, case["src"])
    e_r = R.envelope(case["x"][:-1], case["G"], ref["params"][:-1], win[:-1], None, case["src"])[2]
    bound = np.einsum("dij,dj->di", np.abs(np.linalg.inv(N)), MARGIN * e_r) + 10 * tol * R.scales(ref["params"][:-1])
    diff = np.abs(got[:-1] - ref["params"][:-1])
    print(f"noiseless {frame} K {K}: largest |device - reference| / bound {(diff / bound).max():.3e}; "
          f"largest scaled |device - truth| {(np.abs(got[:-1] - case['truth'][:-1]) / R.scales(case['truth'][:-1])).max():.3e}")
    assert np.all(diff <= bound)
    np.testing.assert_allclose(fit.offsets()[-1], case["nominal"][-1].astype(np.float32), rtol=0, atol=0)
    alone = device_fit(case["x"], slice(0, D - 1))
    assert torch.equal(alone.params, fit.params[:-1]), "the failed detector changed the others"
    if K == 7:
        major, minor, angle = R.fwhm_angle(got[:-1, 3], got[:-1, 4], got[:-1, 5])
        np.testing.assert_allclose(fit.fwhm_major.cpu().numpy()[:-1], major, rtol=1e-12)
        np.testing.assert_allclose(fit.fwhm_minor.cpu().numpy()[:-1], minor, rtol=1e-12)
    else:
        np.testing.assert_allclose(fit.fwhm.cpu().numpy()[:-1], np.sqrt(8 * np.log(2) / got[:-1, 3]), rtol=1e-12)
    # white noise of known sigma
    sigma = 0.02
    noisy = (case["x"].astype(np.float64) + sigma * np.random.default_rng(11).standard_normal(case["x"].shape)).astype(np.float32)
    ref_n = R.lm_fit(lambda p: R.sums(noisy, case["G"], p, win, None, case["src"]), start, n_iter=30, tol=tol)
    sig_ref = np.sqrt(np.einsum("dii->di", ref_n["cov"][:-1]))
    pull_ref = np.abs(ref_n["params"][:-1] - case["truth"][:-1]) / sig_ref
    assert ref_n["ok"][:-1].all() and pull_ref.max() < 5.0, "the reference fit misses the truth on this seed"
    fit_n = device_fit(noisy)
    assert bool(fit_n.ok[:-1].all()) and not bool(fit_n.ok[-1])
    sig = np.sqrt(np.einsum("dii->di", fit_n.cov.cpu().numpy()[:-1]))
    pull = np.abs(fit_n.params.cpu().numpy()[:-1] - case["truth"][:-1]) / sig
    print(f"noisy {frame} K {K}: largest pull {pull.max():.2f} (reference {pull_ref.max():.2f}); chi2 / dof "
          f"{float((fit_n.chi2[:-1] / (fit_n.hits[:-1] - K)).mean()) / sigma**2:.3f}")
    assert pull.max() < 5.0
    np.testing.assert_allclose(fit_n.sigma_dx.cpu().numpy()[:-1], sig[:, 1], rtol=1e-12)


@pytest.fixture(scope="module")
def source_scan(gpu_ctx):
    """Simulation over a ProjectionMap with one Gaussian source six pixels wide at its centre: a daisy of 0.35 degrees over
    an array of 0.3 degrees, 30 positions x 2 bands, 4000 samples, gains scattered by 5 %, the true offsets 0.3 beam
    sigmas off the nominal table.  No noise: what the fit misses is model mismatch (a pixelised source under the
    detector's beam, the three-tap time kernel)."""
    import torch

    from maria_amd import beamfit
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site, compute_angular_fwhm
    from maria_amd.sim import Plan, Simulation, sky_transform_stack

    bands = [Band(center=93e9, width=27e9, shape="top_hat", name="f093", gain_error=0.05),
             Band(center=150e9, width=41e9, shape="top_hat", name="f150", gain_error=0.05)]
    nominal_dets = Detectors.hexagon(30, 0.3, bands, primary_size=6.0)
    nominal = nominal_dets.offsets.copy()
    rng = np.random.default_rng(2)
    plan = Plan.daisy(start_time=1.7e9, duration=80.0, sample_rate=50.0, scan_center=(120.0, 55.0), radius=0.35, speed=0.5)
    site = Site(altitude=5000.0)
    stack = sky_transform_stack(plan.time, site.latitude, site.longitude)
    centre = beamfit.scan_center(plan.phi, plan.theta, stack)
    n, width = 257, 1.2
    src_sigma = np.radians(0.03) / np.sqrt(8 * np.log(2))
    ax = np.radians(width) * np.linspace(-0.5, 0.5, n)
    X, Y = np.meshgrid(ax, ax)
    sky = mmap.ProjectionMap(np.exp(-(X * X + Y * Y) / (2 * src_sigma**2)).astype(np.float32), nu=150e9, width=width, center=np.degrees(centre),
                             frame="ra/dec")
    dets = Detectors.hexagon(30, 0.3, bands, primary_size=6.0)
    beam_sigma = float(np.min(compute_angular_fwhm(fwhm_0=6.0, z=np.inf, nu=dets.band_center))) / np.sqrt(8 * np.log(2))
    truth = nominal + rng.normal(0.0, 0.3 * beam_sigma, nominal.shape)
    dets.offsets = truth.copy()
    (tod,) = Simulation(Instrument(dets), plan, site, map=sky, noise=False, gain_seed=9).run()
    assert tod.units == "K_RJ" and tod.fields == ["map"]
    gain = np.exp(0.05 * np.random.default_rng(9).standard_normal(dets.n))
    x = np.asarray(tod.data["map"].cpu() if isinstance(tod.data["map"], torch.Tensor) else tod.data["map"], np.float32)
    assert x.shape == (60, 4000)
    return dict(tod=tod, x=x, nominal=nominal, truth=truth, gain=gain, centre=centre, stack=stack, bands=bands, band=np.asarray(dets.band_index))


def test_end_to_end_source_scan(gpu_ctx, source_scan):
    """``tod.with_offsets(nominal).fit_beams()`` on a simulated source scan: every detector ok; the fitted offsets closer
    to the truth than the nominal ones for every detector and within a margin of 2 of what the reference fit attains on the
    same TOD (printed: DESIGN 3.29 records it); the relative gains under the same rule; a BinMapper map from the fitted
    table has the higher source peak; and a common mode removed with the source masked leaves the fitted amplitudes closer
    to the unfiltered ones than one removed unmasked."""
    import torch

    from maria_amd import beamfit
    from maria_amd.mappers import BinMapper
    from maria_amd.sim import TOD

    s = source_scan
    tod, nominal, truth = s["tod"], s["nominal"], s["truth"]
    nom = tod.with_offsets(nominal)
    assert nom.data is tod.data and np.array_equal(nom.coords.offsets, nominal) and np.array_equal(tod.coords.offsets, truth)
    fit = nom.fit_beams(ctx=gpu_ctx)
    assert bool(fit.ok.all()), f"not ok: {np.flatnonzero(~fit.ok.cpu().numpy())}"
    # the reference on the same TOD: the same window, the same starting rule
    fwhm = nom.beam_fwhm()
    radius = 3.0 * float(fwhm.max())
    az, el = np.asarray(tod.coords._baz, np.float32), np.asarray(tod.coords._bel, np.float32)
    G = R.rotations(az, el, s["stack"], s["centre"])
    ox, oy = R.offsets(G, nominal[:, 0].astype(np.float32), nominal[:, 1].astype(np.float32))
    win = (ox * ox + oy * oy > radius * radius).astype(np.uint8)
    xin = np.where(win == 0, s["x"].astype(np.float64), np.nan)
    mean, peak = np.nanmean(xin, axis=1), np.nanmax(xin, axis=1)
    start = np.stack([peak - mean, nominal[:, 0].astype(np.float32), nominal[:, 1].astype(np.float32), 8 * np.log(2) / fwhm**2, mean], axis=1)
    ref = R.lm_fit(lambda p: R.sums(s["x"], G, p, win), start, n_iter=20)
    assert ref["ok"].all()
    err = np.hypot(*(fit.offsets() - truth).T)
    err_ref = np.hypot(*(ref["params"][:, 1:3] - truth).T)
    err_nom = np.hypot(*(nominal - truth).T)
    print(f"offsets: device fit misses the truth by at most {err.max():.3e} rad (median {np.median(err):.3e}), the reference by {err_ref.max():.3e}, "
          f"the nominal table by {err_nom.max():.3e} (median {np.median(err_nom):.3e}); beam sigma {float(fwhm.min()) / 2.3548:.3e}")
    assert np.all(err < err_nom)
    assert err.max() <= 2.0 * err_ref.max()
    band = s["band"]
    g_true = np.concatenate([s["gain"][band == b] / np.median(s["gain"][band == b]) for b in (0, 1)])
    g_fit = fit.relative_gain()
    amp_ref = ref["params"][:, 0]
    g_ref = np.concatenate([amp_ref[band == b] / np.median(amp_ref[band == b]) for b in (0, 1)])
    print(f"relative gain: device fit off by at most {np.abs(g_fit - g_true).max():.3e} (median {np.median(np.abs(g_fit - g_true)):.3e}), the "
          f"reference by {np.abs(g_ref - g_true).max():.3e}; injected scatter {np.std(g_true):.3e}")
    assert np.abs(g_fit - g_true).max() <= 2.0 * np.abs(g_ref - g_true).max()
    assert np.median(np.abs(g_fit - g_true)) < 0.2 * np.std(g_true)  # (the largest misses are the mismatch's, the reference's too)
    # a fitted table goes straight into a mapper
    kw = dict(center=np.degrees(s["centre"]), width=0.5, resolution=0.005, stokes="I", nu=[b.center for b in s["bands"]], frame="ra/dec",
              units="K_RJ", degrees=True, device=DEV)
    peaks = {}
    for name, t in (("nominal", nom), ("fitted", tod.with_offsets(fit.offsets()))):
        mapper = BinMapper([t], **kw)
        mapper.run()
        peaks[name] = float(np.nanmax(np.asarray(mapper.map)))
    print(f"source peak in a binned map: nominal table {peaks['nominal']:.5f}, fitted table {peaks['fitted']:.5f}")
    assert peaks["fitted"] > peaks["nominal"]
    # the source mask keeps a common-mode filter honest
    masked = nom.mask_source()
    assert masked.flags is not None and 0.0 < float((masked.flags != 0).float().mean()) < 0.5 and nom.flags is None

    def amplitude_after(t):
        out = t.remove_common_mode(n_iter=1)
        return TOD(out.data, out.dets, out.coords, units=out.units, metadata=out.metadata, flags=None).fit_beams(ctx=gpu_ctx).amplitude.cpu().numpy()

    a_raw = fit.amplitude.cpu().numpy()
    a_masked, a_plain = amplitude_after(masked), amplitude_after(nom)
    print(f"amplitude after a common-mode filter: masked off by {np.nanmax(np.abs(a_masked / a_raw - 1)):.3e}, unmasked by "
          f"{np.nanmax(np.abs(a_plain / a_raw - 1)):.3e} (median {np.nanmedian(np.abs(a_plain / a_raw - 1)):.3e})")
    assert np.all(np.abs(a_masked - a_raw) < np.abs(a_plain - a_raw))
