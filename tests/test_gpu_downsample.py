"""mrx_tod_decimate, maria_amd.downsample.decimate and TOD.downsample on the device, against the formula of
include/mrx.h evaluated in float64 on the float32 inputs.

Tolerance of every kernel comparison: |y - ref| <= 2^-23 |ref| + 1e-12 sum|h| max|x| / min(denominator): one float32
rounding, and slack for the order of the float64 sum."""

import numpy as np
import pytest
import scipy.signal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def reference(x, q, h):
    """(y, denominators) of the formula in float64: the correlation of the zero-padded rows, evaluated at every q-th
    sample, over the same correlation of a row of ones (the taps that meet the row)."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    H, T = (h.size - 1) // 2, x.shape[1]
    windows = lambda v: np.lib.stride_tricks.sliding_window_view(np.pad(v, ((0, 0), (H, H))), h.size, axis=1)[:, ::q]  # noqa: E731
    den = (windows(np.ones((1, T))) @ h)[0]
    return (windows(x) @ h) / den, den


def tolerance(ref, x, h, den):
    return 2.0**-23 * np.abs(ref) + 1e-12 * np.abs(h).sum() * np.abs(x).max() / den.min()


def run(gpu_ctx, x, q, h, pad_x=0, pad_y=0):
    """decimate() of the [D, T] float32 array x held at row pitch T + pad_x, into rows of pitch T_out + pad_y of a buffer
    pre-filled with 7.0; asserts that nothing but the outputs was written and that the input is bit-identical after."""
    import torch

    from maria_amd import downsample

    D, T = x.shape
    T_out = downsample.output_length(T, q)
    ld_x, ld_y = T + pad_x, T_out + pad_y
    xbuf = torch.full((D * ld_x + 64,), -3.0, dtype=torch.float32, device=DEV)
    xv = torch.as_strided(xbuf, (D, T), (ld_x, 1))
    xv.copy_(torch.as_tensor(x))
    before = xbuf.clone()
    ybuf = torch.full((D * ld_y + 64,), 7.0, dtype=torch.float32, device=DEV)
    yv = torch.as_strided(ybuf, (D, T_out), (ld_y, 1))
    out = downsample.decimate(xv, q, taps=h, ctx=gpu_ctx, out=yv)
    torch.cuda.synchronize()
    assert out is yv
    assert torch.equal(xbuf, before), "the input changed"
    y = yv.cpu().numpy()
    yv.fill_(7.0)
    assert bool((ybuf == 7.0).all()), "written past T_out"
    return y


def check(gpu_ctx, x, q, h, **pads):
    y = run(gpu_ctx, x, q, h, **pads)
    ref, den = reference(x, q, h)
    assert y.shape == ref.shape and y.dtype == np.float32
    err = np.abs(y.astype(np.float64) - ref)
    tol = tolerance(ref, x, h, den)
    worst = float((err / tol).max())
    print(f"D {x.shape[0]} T {x.shape[1]} q {q} taps {len(h)}: max |y - ref| / tolerance = {worst:.3f}")
    assert worst <= 1.0
    return y


def noise_rows(D, T, seed=0):
    return (np.random.default_rng(seed).standard_normal((D, T)) + 5).astype(np.float32)


def lowpass(n_taps, q):
    return scipy.signal.firwin(n_taps, 1.0 / q) if n_taps > 1 else np.ones(1)


def tile():
    from maria_amd import downsample

    return downsample.TILE_OUTPUTS


@pytest.mark.parametrize("D,T,q,n_taps,pad_x,pad_y", [
    (1, 1, 2, 1, 0, 0),            # a single sample
    (3, 37, 2, 41, 0, 0),          # T < n_taps: every output truncated on both sides, odd T
    (2, 100, 16, 321, 0, 0),       # T < H
    (5, 1000, 4, 81, 3, 1),        # padded, unaligned rows
    (130, 5000, 4, 81, 0, 0),      # a row count that divides nothing
    (3, 70001, 32, 641, 0, 0),     # the largest factor
    (2, 240000, 8, 161, 0, 0),     # benchmark-length rows, many tiles
])
def test_decimate_matches_the_formula(gpu_ctx, D, T, q, n_taps, pad_x, pad_y):
    check(gpu_ctx, noise_rows(D, T, seed=T), q, lowpass(n_taps, q), pad_x=pad_x, pad_y=pad_y)


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_tile_seams(gpu_ctx, extra):
    """T_out one short of a workgroup's run of outputs, exactly one run, and one more: the seam and the halo across it."""
    from maria_amd import downsample

    T_out = tile() + extra
    T = 8 * T_out - 3
    assert downsample.output_length(T, 8) == T_out
    check(gpu_ctx, noise_rows(4, T, seed=extra + 7), 8, lowpass(161, 8))


def test_one_tap_picks_bit_for_bit(gpu_ctx):
    x = noise_rows(2, 1025, seed=3)
    y = run(gpu_ctx, x, 3, np.array([1.0]))
    np.testing.assert_array_equal(y, x[:, ::3])


def test_asymmetric_taps_fix_the_orientation(gpu_ctx):
    """Random asymmetric taps (all positive: every truncated sum is): a convolution instead of the correlation fails."""
    rng = np.random.default_rng(12)
    h = rng.uniform(0.05, 1.0, 33) * np.linspace(0.2, 2.0, 33)
    x = noise_rows(3, 4001, seed=4)
    y = check(gpu_ctx, x, 5, h)
    flipped, den = reference(x, 5, h[::-1])
    assert np.abs(y - flipped).max() > 100 * tolerance(flipped, x, h, den).max()  # the test can tell the two apart


def test_constant_rows_map_onto_themselves(gpu_ctx):
    c = 23.7
    x = np.full((3, 999), c, np.float32)
    y = check(gpu_ctx, x, 8, lowpass(161, 8))
    assert np.abs(y - np.float32(c)).max() <= np.spacing(np.float32(c))  # one ulp, the truncated edges included


def test_interior_matches_scipy_decimate(gpu_ctx):
    from maria_amd import downsample

    D, T, q = 4, 20000, 8
    x = noise_rows(D, T, seed=9)
    h = downsample.design_taps(q)
    H = (h.size - 1) // 2
    y = run(gpu_ctx, x, q, None)  # taps=None: the default design
    ref = scipy.signal.decimate(x.astype(np.float64), q, ftype="fir", axis=1)
    assert y.shape == ref.shape
    j = np.arange(y.shape[1])
    inner = (j * q >= H) & (j * q < T - H)
    assert inner.sum() > 2000
    _, den = reference(x[:1], q, h)
    err = np.abs(y - ref)[:, inner]
    assert np.all(err <= tolerance(ref, x, h, den)[:, inner])


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves d_y untouched."""
    import torch

    from maria_amd._lib import ptr

    x = torch.zeros((4, 3000), dtype=torch.float32, device=DEV)
    y = torch.full((4, 1500), 7.0, dtype=torch.float32, device=DEV)
    y1 = torch.full((4, 3000), 7.0, dtype=torch.float32, device=DEV)  # what q = 1 would write, were it let through
    h = torch.ones(1027, dtype=torch.float64, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    good = (ptr(x), 3000, 4, 3000, 2, ptr(h), 41, ptr(y), 1500)
    cases = {
        "q 1": (ptr(x), 3000, 4, 3000, 1, ptr(h), 41, ptr(y1), 3000),
        "q 33": (ptr(x), 3000, 4, 3000, 33, ptr(h), 41, ptr(y), 1500),
        "n_taps 40": (ptr(x), 3000, 4, 3000, 2, ptr(h), 40, ptr(y), 1500),
        "n_taps 0": (ptr(x), 3000, 4, 3000, 2, ptr(h), 0, ptr(y), 1500),
        "n_taps 1027": (ptr(x), 3000, 4, 3000, 2, ptr(h), 1027, ptr(y), 1500),
        "D 0": (ptr(x), 3000, 0, 3000, 2, ptr(h), 41, ptr(y), 1500),
        "T 0": (ptr(x), 3000, 4, 0, 2, ptr(h), 41, ptr(y), 1500),
        "ld_x < T": (ptr(x), 2999, 4, 3000, 2, ptr(h), 41, ptr(y), 1500),
        "ld_y < T_out": (ptr(x), 3000, 4, 3000, 2, ptr(h), 41, ptr(y), 1499),
        "y is x": (ptr(y), 1500, 4, 1500, 2, ptr(h), 41, ptr(y), 1500),
        "null x": (None,) + good[1:],
        "null taps": good[:5] + (None,) + good[6:],
        "null y": good[:7] + (None, 1500),
    }
    for name, args in cases.items():
        assert lib.mrx_tod_decimate(hd, *args) == -1, name
        assert b"mrx_tod_decimate" in lib.mrx_last_error(hd), name
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((y1 == 7.0).all())
    assert lib.mrx_tod_decimate(hd, *good) == 0


def hand_tod(D=6, T=3001, fs=200.0, seed=0, gamma=None):
    """A two-field TOD built by hand: one numpy field, one device-tensor field.  ``gamma``: the detectors' polarisation
    angle (None: unpolarised)."""
    import torch

    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t, radius_deg=0.3)
    dets = Detectors(synthetic.hex_pack(D, np.radians(0.4)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int),
                     gamma=None if gamma is None else np.full(D, float(gamma)))
    rng = np.random.default_rng(seed)
    data = {"map": (rng.standard_normal((D, T)) + 5).astype(np.float32),
            "noise": torch.as_tensor(rng.standard_normal((D, T)).astype(np.float32)).to(DEV)}
    tod = TOD(data, dets, Coordinates(t, az, el, offsets=dets.offsets), units="K_RJ", metadata={"latitude": -23.0, "longitude": -67.8})
    return tod, float(np.degrees(az.mean())), float(np.degrees(el.mean()))


def test_tod_downsample(gpu_ctx):
    import torch

    from maria_amd import downsample

    tod, _, _ = hand_tod()
    D, T, q = 6, 3001, 4
    kept = {k: (v.clone() if isinstance(v, torch.Tensor) else v.copy()) for k, v in tod.data.items()}
    t0, az0, el0 = tod.coords.t.copy(), tod.coords._baz.copy(), tod.coords._bel.copy()
    tod._calibrator = lambda data, to_krj: data  # a TOD that could convert units
    low = tod.downsample(q, ctx=gpu_ctx)
    assert low is not tod and low.fields == tod.fields == ["map", "noise"]
    T_out = downsample.output_length(T, q)
    h = downsample.design_taps(q)
    for name in low.fields:
        v = low.data[name]
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (D, T_out)
        x = kept[name].cpu().numpy() if isinstance(kept[name], torch.Tensor) else kept[name]
        ref, den = reference(x, q, h)
        assert np.all(np.abs(v.cpu().numpy() - ref) <= tolerance(ref, x, h, den))
    np.testing.assert_array_equal(low.coords.t, t0[::q])
    np.testing.assert_array_equal(low.coords._baz, az0[::q])
    np.testing.assert_array_equal(low.coords._bel, el0[::q])
    assert low.coords.t.shape == (T_out,)
    np.testing.assert_array_equal(low.coords.offsets, tod.coords.offsets)
    assert low.dets is tod.dets and low.units == tod.units == "K_RJ"
    assert low.metadata["latitude"] == -23.0 and low.metadata["longitude"] == -67.8
    ds = low.metadata["downsample"]
    assert ds["factor"] == q and ds["n_taps"] == h.size and ds["sample_rate"] == pytest.approx(50.0, rel=1e-6)
    # the source is as it was
    assert "downsample" not in tod.metadata and tod.fields == ["map", "noise"]
    for name, v in kept.items():
        same = torch.equal(tod.data[name], v) if isinstance(v, torch.Tensor) else np.array_equal(tod.data[name], v)
        assert same, name
    np.testing.assert_array_equal(tod.coords.t, t0)
    assert tod.to("pW") is not None  # the source converts ...
    with pytest.raises(NotImplementedError):  # ... the downsampled TOD carries no calibrator
        low.to("pW")


def test_bin_mapper_takes_a_downsampled_tod_exactly(gpu_ctx):
    """BinMapper (stokes "I", nearest) on tod.downsample(4) against BinMapper on a TOD built by hand from the float64
    reference of the same decimation (rounded to float32) and the picked pointing, 31 detectors x 8001 samples: the
    weight maps are equal bit for bit, and the maps agree within 2 * 2^-23 * max|tod| (a map pixel is an average with
    non-negative weights of samples, each off by at most one float32 rounding).

    The detectors have polarisation angle 0: their I weight (map.mueller_row) is exactly 1 / 2, so every weight is an exact
    float64 sum whatever order the binning adds it in (as tests/test_gpu_map_routed.py's dyadic inputs).  An unpolarised
    detector's is 0.5 * sqrt(2) * sqrt(2) = 1 + 2^-52, and sums of that round differently in different orders."""
    from maria_amd import downsample
    from maria_amd.map import mueller_row
    from maria_amd.mappers import BinMapper
    from maria_amd.sim import TOD, Coordinates

    q = 4
    tod, az, el = hand_tod(D=31, T=8001, seed=5, gamma=0.0)
    assert np.all(mueller_row(tod.dets.gamma)[:, 0] == 0.5)  # the premise of the bit-for-bit comparison
    tod.data = {"map": tod.data["map"]}
    ref, _ = reference(tod.data["map"], q, downsample.design_taps(q))
    c = tod.coords
    by_hand = TOD({"map": ref.astype(np.float32)}, tod.dets, Coordinates(c.t[::q], c._baz[::q], c._bel[::q], offsets=c.offsets),
                  units="K_RJ", metadata=dict(tod.metadata))
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="I", frame="az/el", units="K_RJ")
    a = BinMapper([tod.downsample(q, ctx=gpu_ctx)], **kw)
    b = BinMapper([by_hand], **kw)
    ma, mb = a.run().data, b.run().data
    wa, wb = a.products["weight"], b.products["weight"]
    np.testing.assert_array_equal(wa, wb)
    np.testing.assert_array_equal(wa, 0.5 * np.rint(2 * wa))  # half the hit counts
    assert wa.sum() > 0.5 * 0.5 * 31 * ref.shape[1]  # most samples fall on the map
    np.testing.assert_array_equal(np.isnan(ma), np.isnan(mb))
    ok = np.isfinite(mb)
    assert ok.sum() > 100
    err = np.abs(ma[ok].astype(np.float64) - mb[ok]).max()
    bound = 2 * 2.0**-23 * np.abs(ref).max()
    print(f"max |map - map of the reference| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def _centre(az, el, transform):
    """Centre of the scanned patch in the map's frame."""
    from oracle import mapsample

    phi, theta = mapsample.frame_angles(az[None, :], el[None, :], transform)
    xyz = mapsample.phi_theta_to_xyz(phi[0], theta[0]).astype(float).mean(axis=0)
    xyz /= np.linalg.norm(xyz)
    return float(np.arctan2(xyz[1], xyz[0]) % (2 * np.pi)), float(np.arcsin(xyz[2]))


def test_recover_map_at_the_reduced_rate(gpu_ctx):
    """The reference's map-recovery bound (maria/tests/map/test_recover_map.py:15-69, test_gpu_map.py's set-up: 300
    positions x 3 bands behind a beam-free dish, a 60 s daisy, no noise, no atmosphere) with the TOD simulated at 200 Hz
    and binned from tod.downsample(4) on the input map's own grid: per band, sqrt(nansum(w (m1 - m0)^2) / nansum(w))
    < 1e-3 K_RJ, and, as there, below 1 % of the map's peak.  The residual is
    printed beside that of the same simulation made directly at 50 Hz (DESIGN 3.19 holds both)."""
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.mappers import BinMapper
    from maria_amd.sim import Plan, Simulation, sky_transform_stack

    bands = [Band(center=90e9, width=30e9, name="f090"), Band(center=150e9, width=40e9, name="f150"), Band(center=220e9, width=50e9, name="f220")]
    n, width = 128, 1.0  # degrees
    res = width / (n - 1)
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    rng = np.random.default_rng(8)
    field = np.fft.irfft2(np.fft.rfft2(rng.standard_normal((n, n))) * np.exp(-0.5 * (np.hypot(*np.meshgrid(np.fft.rfftfreq(n), np.fft.fftfreq(n))) * 12.0) ** 2), s=(n, n))
    data = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0 + 4e-4 * field / field.std()
    data = (data - data.mean()).astype(np.float32)
    inst = Instrument(Detectors.hexagon(300, width / 2, bands, primary_size=1000.0))
    site = Site(altitude=5190.0)
    residual = {}
    for rate, q in ((200.0, 4), (50.0, 1)):
        plan = Plan.daisy(start_time=1.7e9, duration=60.0, sample_rate=rate, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
        centre = _centre(plan.phi.astype(np.float32), plan.theta.astype(np.float32), sky_transform_stack(plan.time, site.latitude, site.longitude))
        sky = mmap.ProjectionMap(data, nu=150e9, width=width, center=np.degrees(centre), frame="ra/dec")
        (tod,) = Simulation(inst, plan, site, map=sky, noise=False).run()
        assert tod.units == "K_RJ" and set(tod.fields) == {"map"}
        if q > 1:
            tod = tod.downsample(q, ctx=gpu_ctx)
            assert tod.coords.t.size == 3000
        mapper = BinMapper([tod], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="I",
                           nu=[b.center for b in bands], frame="ra/dec", units="K_RJ")
        out = mapper.run()
        assert out.data.shape[-2:] == (n, n) and np.allclose(out.xi, sky.xi, atol=1e-12) and np.allclose(out.eta, sky.eta, atol=1e-12)
        m0, m1 = sky.data[0, 0], out.data[0, :]
        w = mapper.products["weight"][0, -1]
        assert (w > 0).mean() > 0.5
        residual[rate] = np.sqrt(np.nansum(w * (m1 - m0) ** 2, axis=(-1, -2)) / np.nansum(w))
    print("weighted rms residual per band [K_RJ]: 200 Hz downsampled by 4", residual[200.0], "simulated at 50 Hz", residual[50.0])
    assert residual[200.0].shape == (3,) and np.all(residual[200.0] < 1e-3)  # the reference's assertion
    assert np.all(residual[200.0] < 0.01 * np.abs(data).max())               # ... and one that a 5-mK map can fail


def test_the_filter_path_takes_a_downsampled_tod(gpu_ctx):
    """MaximumLikelihoodMapper(noise_model=...) on tod.downsample(4) of a small noisy simulation (61 positions, 200 Hz,
    60 s): it runs, converges, and the map is finite exactly where the block solve's mask is set (the white-noise map's
    finite pixels).  Plumbing, not an accuracy claim."""
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.mappers import MaximumLikelihoodMapper
    from maria_amd.sim import Plan, Simulation, sky_transform_stack

    band = Band(center=150e9, width=30e9, name="f150", NEP=3e-17, knee=1.0)
    inst = Instrument(Detectors.hexagon(61, 0.4, [band], primary_size=12.0))
    plan = Plan.daisy(start_time=1.7e9, duration=60.0, sample_rate=200.0, scan_center=(120.0, 55.0), radius=0.25, speed=0.5)
    site = Site(altitude=5190.0)
    centre = _centre(plan.phi.astype(np.float32), plan.theta.astype(np.float32), sky_transform_stack(plan.time, site.latitude, site.longitude))
    n = 64
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    sky = mmap.ProjectionMap((1e-3 * np.exp(-(X**2 + Y**2) / 0.1)).astype(np.float32), nu=150e9, width=1.0, center=np.degrees(centre), frame="ra/dec")
    (tod,) = Simulation(inst, plan, site, map=sky, noise=True, noise_seed=3).run()
    low = tod.downsample(4, ctx=gpu_ctx)
    assert low.coords.t.size == 3000 and set(low.fields) == {"map", "noise"}
    noise = low.data["noise"].cpu().numpy().astype(np.float64)
    white = 2.0 * np.median(np.var(np.diff(noise, axis=1), axis=1) / 2) / 50.0  # one-sided level, signal units^2 / Hz
    assert np.isfinite(white) and white > 0
    kw = dict(center=np.degrees(centre), width=0.8, resolution=1.0 / 30, stokes="I", nu=[150e9], frame="ra/dec", units="K_RJ",
              tol=1e-6, max_iter=300)
    gls = MaximumLikelihoodMapper([low], noise_model={"white": white, "knee": 1.0, "alpha": 1.0}, **kw)
    m = gls.run().data
    assert gls.products["converged"], gls.products["residuals"]
    assert gls.products["noise_filter"][0]["K"] == 2048  # the default, min(2048, T - 1) lags: at 50 Hz four times the seconds
    solved = np.isfinite(MaximumLikelihoodMapper([low], **kw).run().data)
    assert solved.mean() > 0.3
    np.testing.assert_array_equal(np.isfinite(m), solved)
