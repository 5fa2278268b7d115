"""The CMB field on the device: mrx_cmb_generate against the float64 rebuild of tests/cmb_ref.py draw for
draw and in its statistics, and Simulation(cmb=...) against the map path, the oracle and the half-wave-plate formula."""

import numpy as np
import pytest

import cmb_ref
import hwp_ref

pytestmark = pytest.mark.gpu

ARCMIN = np.radians(1.0 / 60.0)


def _fields(ctx, seed, stream, ny, nx, res, table, out_shape=None):
    from maria_amd import cmb

    return cmb.generate_fields(ctx, seed, stream, ny, nx, res, table, out_shape).cpu().numpy()


_REFS = {}


def _reference(seed, stream, ny, nx, res, table):
    """The float64 rebuild, made once per case and left as it is."""
    from maria_amd._lib import philox4x32

    key = (seed, stream, ny, nx)
    if key not in _REFS:
        g = cmb_ref.philox_normals(philox4x32, seed, stream, ny, nx)
        P = cmb_ref.half_spectra(g, ny, nx, res, table)
        ref = cmb_ref.fields(P, ny, nx)
        for a in (g, P, ref):
            a.setflags(write=False)
        _REFS[key] = (g, P, ref)
    return _REFS[key]


# (64, 2048) beside the issue's four: the only one whose rows take the register form of pass 2 (nx >= 2048)
@pytest.mark.parametrize("ny,nx,out", [(64, 128, None), (128, 64, None), (1024, 64, None), (64, 1024, None), (64, 2048, None),
                                       (128, 64, (100, 60))])
def test_draw_for_draw(gpu_ctx, ny, nx, out):
    """T, Q and U against the reference on the same Philox cells, within test_screen_fft_matches_numpy_irfft's
    2e-5 max|ref| per field (the same transforms; the float32 rotation and interpolation add ulps per cell): the Stockham
    and the register forms of both passes, a table that ends inside the domain's corners (cells beyond its last row),
    B modes present (r = 0.05), and a written block smaller than the domain.  On the self-mirrored column kx = 0 the
    symmetrisation of Q is minus that of E and T's is T's own, so the T-E covariance survives it: checked on the
    reference's modes, which the device's fields then match."""
    from maria_amd import cmb

    res = 4 * ARCMIN
    table = cmb.spectrum_table(cmb.toy_spectrum(3000, r=0.05), nx * res, ny * res)
    assert np.pi * np.sqrt(2) / res > 3000 > np.pi / res  # the table ends between the Nyquist frequency and the corner
    g, P, ref = _reference(17, 3, ny, nx, res, table)
    oy, ox = out or (ny, nx)
    got = _fields(gpu_ctx, 17, 3, ny, nx, res, table, out)
    assert got.shape == (3, oy, ox) and np.isfinite(got).all()
    for f, name in enumerate("TQU"):
        err, peak = np.abs(got[f] - ref[f, :oy, :ox]).max(), np.abs(ref[f]).max()
        print(f"{name} {ny}x{nx}: max error {err / peak:.2e} of max|ref|")
        assert peak > 0 and err <= 2e-5 * peak, name
    # kx = 0: cos 2 phi = -1, sin 2 phi = 0
    ell, _, _ = cmb_ref.rotation(ny, nx, res)
    cT, cTE, cE, cB = cmb_ref.coefficients(table, ell)
    E = cTE * g[0] + cE * g[1]
    E[cmb_ref.nyquist_mask(ny, nx)] = 0.0
    col, half = E[:, 0], ny // 2
    sym = np.zeros(ny, complex)
    sym[1:half] = (col[1:half] + np.conj(col[:half:-1])) / np.sqrt(2)
    sym[:half:-1] = np.conj(sym[1:half])
    assert np.abs(sym).max() > 0
    np.testing.assert_allclose(P[1][:, 0], -sym, atol=1e-14 * np.abs(sym).max())


def test_statistics(gpu_ctx):
    """256^2 at 2' pixels, bins of 200 from ell = 100 that hold N >= 400 independent cells of the half plane (at least 15
    of them): TT and EE within 5 / sqrt N of the input, TE within 5 sqrt((C_TT C_EE + C_TE^2) / 2N); and with C_BB = 0 the
    B power over the full plane is below 1e-8 of E's -- which fails if a Nyquist line carries power
    (tests/test_host_cmb.py shows that on the reference)."""
    from maria_amd import cmb

    ny = nx = 256
    res = 2 * ARCMIN
    table = cmb.spectrum_table(cmb.toy_spectrum(9000), nx * res, ny * res)
    tqu = _fields(gpu_ctx, 21, 0, ny, nx, res, table)
    bins = cmb_ref.binned(tqu, res, table)
    assert len(bins) >= 15 and min(b["N"] for b in bins) > 400
    for b in bins:
        print({k: (round(v, 6) if isinstance(v, float) and abs(v) > 1e-3 else v) for k, v in b.items()})
        assert abs(b["tt"] - 1) <= 5 / np.sqrt(b["N"]), b
        assert abs(b["ee"] - 1) <= 5 / np.sqrt(b["N"]), b
        assert abs(b["te"] - b["c_te"]) <= 5 * np.sqrt(b["var_te"] / b["N"]), b
    ratio = cmb_ref.b_to_e(tqu, res)
    print(f"sum |B|^2 / sum |E|^2 = {ratio:.3e}")
    assert ratio <= 1e-8


def test_reproducible_and_apart_from_the_screens(gpu_ctx):
    import torch

    from maria_amd import cmb
    from maria_amd._lib import ptr

    ny = nx = 128
    res = 3 * ARCMIN
    table = cmb.spectrum_table(cmb.toy_spectrum(6000, r=0.1), nx * res, ny * res)

    def screen():
        out = torch.empty((ny, nx), dtype=torch.float32, device="cuda:0")
        work = torch.empty(((ny + 16) * (nx // 2 + 1), 2), dtype=torch.float32, device="cuda:0")
        gpu_ctx.call("mrx_screen_generate", 7, 2, ny, nx, 5.0, 5.0, 100.0, 5.0 / 6.0, ptr(out), ptr(work))
        return out.cpu().numpy()

    before = screen()
    a = _fields(gpu_ctx, 7, 2, ny, nx, res, table)
    after = screen()
    b = _fields(gpu_ctx, 7, 2, ny, nx, res, table)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(before.view(np.uint32), after.view(np.uint32))
    for other in (_fields(gpu_ctx, 8, 2, ny, nx, res, table), _fields(gpu_ctx, 7, 3, ny, nx, res, table)):
        for f in range(3):  # another draw: ||a - b||^2 is 2 ||a||^2 in the mean (a red spectrum holds few modes: no tight bound)
            assert np.linalg.norm(a[f] - other[f]) > 0.5 * np.linalg.norm(a[f])
    # same seed and stream as the screen, another counter tag: T is not the screen over again
    assert abs(np.corrcoef(a[0].ravel(), before.ravel())[0, 1]) < 0.5


def test_entry_refusals(gpu_ctx):
    from maria_amd import cmb
    from maria_amd._lib import MrxError

    table = cmb.spectrum_table(cmb.toy_spectrum(500), 0.1, 0.1)
    with pytest.raises(MrxError, match="powers of two"):
        _fields(gpu_ctx, 1, 0, 96, 64, ARCMIN, table)
    with pytest.raises(MrxError, match="larger than the FFT domain"):
        _fields(gpu_ctx, 1, 0, 64, 64, ARCMIN, table, (65, 64))
    with pytest.raises(MrxError, match="pixel size"):
        _fields(gpu_ctx, 1, 0, 64, 64, 0.0, table)
    with pytest.raises(MrxError, match="rows"):
        _fields(gpu_ctx, 1, 0, 64, 64, ARCMIN, table[:1])


# ---- the front end ------------------------------------------------------------------------------------------------

CENTER = (120.0, 55.0)


def _instrument(n_pos=32, fov=0.4, gamma=None, **band_kw):
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors, Instrument

    bands = [Band(center=93e9, width=27e9, shape="top_hat", name="f093", **band_kw), Band(center=150e9, width=41e9, shape="top_hat", name="f150", **band_kw)]
    pos = synthetic.hex_pack(n_pos, np.radians(fov))
    if gamma is None:
        gamma = np.radians([0.0, 45.0, 90.0, 135.0])[np.arange(2 * n_pos) % 4]
    return Instrument(Detectors(np.tile(pos, (2, 1)), bands, np.repeat(np.arange(2), n_pos), primary_size=6.0, gamma=gamma))


def _plan(duration=60.0):
    from maria_amd.sim import Plan

    return Plan.daisy(start_time=1.7e9, duration=duration, sample_rate=50.0, scan_center=CENTER, radius=0.3, speed=0.3)


@pytest.fixture(scope="module")
def patch(gpu_ctx):
    """A 128^2 IQU CMB in the az/el frame around the scan's centre, 0.01 degrees a pixel."""
    from maria_amd import cmb

    c = cmb.CMB.generate(center=CENTER, width=1.27, resolution=0.01, spectrum=cmb.toy_spectrum(6000, r=0.1), seed=12, frame="az/el", ctx=gpu_ctx)
    assert c.data.shape == (3, 1, 128, 128) and c.units == "K_CMB" and c.seed == 12 and c.stokes == "IQU"
    assert 2e-5 < c.data[0].std() < 3e-4 and 0 < c.data[1].std() < 0.3 * c.data[0].std()  # tens of uK, a few percent polarised
    return c


def _as_krj_map(c):
    """The same numbers as a K_RJ ProjectionMap (the parity flip undone: ProjectionMap flips what it is handed)."""
    from maria_amd.map import ProjectionMap

    data = c.data[:, :, ::-1].copy()
    return ProjectionMap(data, nu=150e9, stokes=c.stokes, resolution=float(np.degrees(c.x_res)), center=np.degrees(c.center), frame=c.frame)


def test_the_field_against_the_map_path(gpu_ctx, patch):
    """No atmosphere, 64 polarised detectors in two bands: the "cmb" field is the "map" field of the same numbers taken
    as K_RJ, times the band's Int tau g dnu / Int tau dnu (float64), within 1e-6 max -- the same float32 chain with another
    constant -- in pW and in K_RJ; with map= and cmb= in one run both fields are those of the separate runs, bit for bit."""
    from maria_amd import cmb
    from maria_amd.sim import Simulation
    from maria_amd.instrument import Site

    inst, plan, site = _instrument(), _plan(), Site(altitude=5190.0)
    sky = _as_krj_map(patch)
    ratio = np.array([np.trapezoid(b.passband(b.nu) * cmb.kcmb_weight(b.nu), x=b.nu) / np.trapezoid(b.passband(b.nu), x=b.nu)
                      for b in inst.dets.bands])[inst.dets.band_index][:, None]
    assert 0.5 < ratio.min() < ratio.max() < 0.9
    both = Simulation(inst, plan, site, map=sky, cmb=patch, noise=False)
    for units in ("pW", "K_RJ"):
        (tc,) = Simulation(inst, plan, site, cmb=patch, noise=False).run(units=units)
        (tm,) = Simulation(inst, plan, site, map=sky, noise=False).run(units=units)
        assert tc.fields == ["cmb"] and tm.fields == ["map"] and tc.units == units
        got, want = tc.data["cmb"].astype(np.float64), tm.data["map"].astype(np.float64) * ratio
        assert got.shape == (64, 3000) and np.abs(want).max() > 0
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{units}: max |cmb - ratio map| = {err:.2e} of max")
        assert err <= 1e-6
        (tb,) = both.run(units=units)
        assert tb.fields == ["map", "cmb"]
        assert np.array_equal(tb.data["cmb"].view(np.uint32), tc.data["cmb"].view(np.uint32))
        assert np.array_equal(tb.data["map"].view(np.uint32), tm.data["map"].view(np.uint32))


def _centre(az, el, transform):
    from oracle import mapsample

    phi, theta = mapsample.frame_angles(az[None, :], el[None, :], transform)
    xyz = mapsample.phi_theta_to_xyz(phi[0], theta[0]).astype(float).mean(axis=0)
    xyz /= np.linalg.norm(xyz)
    return float(np.arctan2(xyz[1], xyz[0]) % (2 * np.pi)), float(np.arcsin(xyz[2]))


def test_with_an_atmosphere_against_the_oracle(gpu_ctx):
    """tod.data["cmb"] in pW against oracle/mapsample fed the same smoothed patch, coarse pwv and the g-weighted
    transmission tables Int tau(nu) g(nu) exp(-opacity) dnu, within test_map_sampling_with_atmospheric_transmission's bound
    (float32 angle rounding times the steepest gradient, + 2e-6 max|ref|; that test's further clause, that the bound is
    below 3e-4 of ITS blob map's peak, is printed here: a CMB's gradients are what they are); in the default units the
    field leaves the sampler in K_RJ (mrx_map_sample_krj) and equals the pW field through TOD.to("K_RJ") bit for bit."""
    from maria_amd import cmb
    from maria_amd.instrument import Site, compute_angular_fwhm
    from maria_amd.sim import Simulation, sky_transform_stack
    from oracle import hotpath, mapsample

    inst, plan = _instrument(n_pos=10, fov=0.25), _plan(duration=40.0)
    site = Site(altitude=1000.0, latitude=-23.0, longitude=-67.8)
    transform = sky_transform_stack(plan.time, site.latitude, site.longitude)
    az32, el32 = plan.phi.astype(np.float32), plan.theta.astype(np.float32)
    centre = _centre(az32, el32, transform)
    sky = cmb.CMB.generate(center=np.degrees(centre), width=1.4, resolution=0.02, spectrum=cmb.toy_spectrum(6000, r=0.1), seed=3, ctx=gpu_ctx)
    kw = dict(atmosphere="2d", atmosphere_kwargs={"n_layers": 2, "seed": 5}, cmb=sky, noise=False)
    sim = Simulation(inst, plan, site, **kw)
    (tod,) = sim.run(units="pW")
    assert set(tod.fields) == {"atmosphere", "cmb"}
    got = tod.data["cmb"]
    obs = sim.obs_list[0]
    atm, dets = obs.atmosphere, inst.dets
    path = atm._device_path()
    coarse = path.coarse_pwv().cpu().numpy()  # [D, Ta]
    ta = path.ta0 + path.dta * np.arange(coarse.shape[1])
    az_d, el_d = hotpath.broadcast(obs.coords.offsets, az32, el32)
    ref = np.zeros_like(got)
    sp = atm.spectrum
    peak_table = 0.0
    for b, band in enumerate(dets.bands):
        rows = np.nonzero(dets.band_index == b)[0]
        fwhm = float(compute_angular_fwhm(fwhm_0=dets.primary_size.mean(), z=np.inf, nu=band.center))
        sigma_pix = fwhm / np.sqrt(8 * np.log(2)) / abs(sky.x_res)
        smoothed = hotpath.map_smooth(sky.data, None, sigma_pix, sigma_pix)
        smoothed = np.asarray(smoothed[0] if isinstance(smoothed, tuple) else smoothed, np.float32)
        nu = sp.side_nu
        tab = np.trapezoid(band.passband(nu) * cmb.kcmb_weight(nu) * np.exp(-sp._opacity), x=nu, axis=-1)
        peak_table = max(peak_table, float(tab.max()))
        ref[rows] = mapsample.sample_maps(az_d[rows], el_d[rows], plan.time, ta, coarse[rows], sky.eta, sky.xi, sky.center,
                                          np.swapaxes(smoothed, 0, 1), mapsample.mueller_row(dets.gamma[rows])[:, :3], cal_tables=[tab],
                                          cal_axes=(sp.side_base_temperature, sp.side_zenith_pwv, sp.side_elevation),
                                          base_temperature=atm.weather.temperature[0], transform_stack=transform)
    grad = max(np.abs(np.diff(sky.data, axis=-1)).max() / abs(sky.xi[1] - sky.xi[0]), np.abs(np.diff(sky.data, axis=-2)).max() / abs(sky.eta[1] - sky.eta[0]))
    bound = 2 * 6e-7 * grad * 1.0 * 1e12 * mapsample.K_B * peak_table  # sum |Mueller row| = 1/2 (1 + |cos| + |sin|) <= 1.21: Q, U << I
    err, peak = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"max |cmb - oracle| = {err:.3e}, bound {bound + 2e-6 * peak:.3e} ({bound / peak:.2e} + 2e-6 of max|ref| = {peak:.3e})")
    assert np.isfinite(got).all() and np.isfinite(ref).all() and peak > 0
    assert err <= bound + 2e-6 * peak
    (tod2,) = Simulation(inst, plan, site, **kw).run()
    assert tod2.units == "K_RJ"
    np.testing.assert_array_equal(tod2.data["cmb"], tod.to("K_RJ").data["cmb"])


def test_generate_covers_every_sample_and_shards_agree(gpu_ctx):
    """cmb="generate" without center / width: one patch for both plans that no sample of any detector leaves (from the
    coordinates, through the oracle's float32 chain); a shard's rows are the unsharded run's, bit for bit; a shard
    without a seed is refused; a run without cmb has no "cmb" field."""
    from maria_amd.instrument import Site
    from maria_amd.sim import Plan, Simulation, sky_transform_stack
    from oracle import hotpath, mapsample

    inst, site = _instrument(), Site(altitude=5190.0)
    plans = [_plan(duration=30.0), Plan.daisy(start_time=1.7e9 + 600.0, duration=30.0, sample_rate=50.0, scan_center=(121.0, 55.5), radius=0.4, speed=0.4)]
    kw = dict(cmb="generate", cmb_kwargs={"resolution": 0.02, "seed": 4}, noise=False)
    sim = Simulation(inst, plans, site, **kw)
    sky = sim.cmb
    assert sky.units == "K_CMB" and sky.seed == 4 and sky.frame == "ra/dec"
    for obs in sim.obs_list:
        t = obs.coords.t
        az_d, el_d = hotpath.broadcast(obs.coords.offsets, obs.boresight._baz.astype(np.float32), obs.boresight._bel.astype(np.float32))
        ox = mapsample.phi_theta_to_offsets(*mapsample.frame_angles(az_d, el_d, sky_transform_stack(t, site.latitude, site.longitude)), *sky.center)
        assert sky.xi.min() < ox[..., 0].min() and ox[..., 0].max() < sky.xi.max()
        assert sky.eta.min() < ox[..., 1].min() and ox[..., 1].max() < sky.eta.max()
        assert max(np.abs(ox[..., 0]).max() / sky.xi.max(), np.abs(ox[..., 1]).max() / sky.eta.max()) > 0.5  # and no far larger than needed
    whole = sim.run(units="pW")
    assert all(t.fields == ["cmb"] and np.isfinite(t.data["cmb"]).all() and np.abs(t.data["cmb"]).max() > 0 for t in whole)
    for rank in range(2):
        part = Simulation(inst, plans, site, shard=(rank, 2), **kw).run(units="pW")
        for w, p in zip(whole, part):
            lo, hi = p.metadata["shard"]["rows"]
            assert hi - lo == 32 and np.array_equal(p.data["cmb"].view(np.uint32), w.data["cmb"][lo:hi].view(np.uint32))
    with pytest.raises(ValueError, match="seed"):
        Simulation(inst, plans, site, shard=(0, 2), cmb="generate", cmb_kwargs={"resolution": 0.02}, noise=False)
    with pytest.raises(TypeError):
        Simulation(inst, plans, site, cmb=_as_krj_map(sky), noise=False)  # a K_RJ map is no CMB
    (plain,) = Simulation(inst, plans[0], site, map=_as_krj_map(sky), noise=False).run(units="pW")
    assert plain.fields == ["map"]


def test_the_field_behind_a_half_wave_plate(gpu_ctx, patch):
    """hwp= with cmb=: the field is S_I + S_c cos 4 chi + S_s sin 4 chi (tests/hwp_ref.py) of the CMB -- S_I from a run
    without a plate on its I plane, S_c and S_s from runs on its Q and U planes with gamma replaced by -gamma and
    pi / 4 - gamma -- within 2^-23 (|S_I| + |S_c| + |S_s|)."""
    from maria_amd import cmb, hwp
    from maria_amd.instrument import Site
    from maria_amd.sim import Simulation

    site, plan = Site(altitude=5190.0), _plan(duration=20.0)
    gamma = np.radians([0.0, 45.0, 90.0, 135.0, 20.0])[np.arange(64) % 5]
    plate = hwp.HWP(frequency=2.0, phase=0.3)

    def planes(keep):
        data = patch.data[:, :, ::-1].copy()
        for i, s in enumerate("IQU"):
            if s not in keep:
                data[i] = 0.0
        return cmb.CMB(data, resolution=0.01, center=np.degrees(patch.center), frame=patch.frame)

    def run(g, sky, **kw):
        (tod,) = Simulation(_instrument(gamma=g), plan, site, cmb=sky, noise=False, **kw).run(units="pW")
        return tod

    turned = run(gamma, patch, hwp=plate)
    assert turned.fields == ["cmb"] and turned.metadata["hwp"]["frequency"] == 2.0
    s_i = run(gamma, planes("I")).data["cmb"]
    s_c = run(-gamma, planes("QU")).data["cmb"]
    s_s = run(np.pi / 4 - gamma, planes("QU")).data["cmb"]
    assert min(np.abs(s).max() for s in (s_i, s_c, s_s)) > 0
    want = hwp_ref.modulate(s_i, s_c, s_s, hwp.carrier(plate.angle(turned.coords.t)))
    err = np.abs(turned.data["cmb"].astype(np.float64) - want)
    tol = 2.0**-23 * (np.abs(s_i) + np.abs(s_c) + np.abs(s_s)).astype(np.float64)
    print(f"max |cmb field - (S_I + S_c cos + S_s sin)| / tol = {(err[tol > 0] / tol[tol > 0]).max():.3f}")
    assert np.all(err <= tol)
