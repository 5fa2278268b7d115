"""GPU tests of the screen side: Gaussian stencil vs scipy, map smoothing, the
Philox generator and the statistics of generated screens."""

import numpy as np
import pytest
import scipy.ndimage
import scipy.stats

from helpers import rel_err

pytestmark = pytest.mark.gpu


def _smooth(ctx, a, sy, sx, truncate=4.0, inplace=False):
    import torch

    from maria_amd._lib import ptr

    d_in = torch.as_tensor(np.ascontiguousarray(a, np.float32)).to("cuda:0")
    d_out = d_in if inplace else torch.empty_like(d_in)
    d_tmp = torch.empty_like(d_in)
    ny, nx = a.shape
    ctx.call("mrx_gauss_smooth2d", ptr(d_in), ptr(d_out), ptr(d_tmp), ny, nx, float(sy), float(sx), float(truncate))
    return d_out.cpu().numpy()


@pytest.mark.parametrize(
    "shape,sy,sx",
    [
        ((128, 128), 4.2, 4.2),
        ((300, 77), 2.0, 7.5),
        ((77, 300), 11.0, 0.6),
        ((64, 64), 0.0, 3.0),  # scipy skips an axis with sigma 0
        ((64, 64), 3.0, 0.0),
        ((5, 9), 3.0, 3.0),  # radius larger than the array: multiple reflections
        ((1, 200), 2.0, 2.0),
        ((513, 1025), 1.3, 25.0),
        ((700, 333), 20.0, 3.0),   # a wide stencil along y on a plane that is not square: the transposed route (radius >= 64)
        ((130, 515), 17.0, 0.0),   # ... alone (no x pass), radius beyond half the plane's height
    ],
)
def test_gauss_matches_scipy(gpu_ctx, shape, sy, sx):
    """scipy.ndimage.gaussian_filter on float32 input: float64 accumulation, float32
    storage between the passes, reflect boundary, radius int(4 sigma + 0.5)
    (atmosphere/atmosphere.py:341-344).  Both accumulation modes (MRX_OPT_GAUSS_ACCUM): the exact one -- scipy's float64
    arithmetic in another order: float32 roundings of the result, <= 2.5e-7 -- and the blocked one (float32 sums over 16
    taps, those in float64: the default from radius 16 on) at <= 1e-6, ten times inside the north star's 1e-5."""
    from maria_amd import _lib

    rng = np.random.default_rng(1)
    a = rng.standard_normal(shape).astype(np.float32)
    ref = scipy.ndimage.gaussian_filter(a, sigma=(sy, sx))
    scale = max(1.0, np.abs(ref).max())
    for mode, bound in ((1, 2.5e-7), (2, 1.0e-6), (0, 1.0e-6)):
        gpu_ctx.set_option(_lib.OPT_GAUSS_ACCUM, mode)
        try:
            got = _smooth(gpu_ctx, a, sy, sx)
            got2 = _smooth(gpu_ctx, a, sy, sx, inplace=True)
        finally:
            gpu_ctx.set_option(_lib.OPT_GAUSS_ACCUM, 0)
        assert got.dtype == np.float32
        assert np.abs(got - ref).max() <= bound * scale, (mode, np.abs(got - ref).max() / scale)
        assert np.array_equal(got, got2)
        if mode == 0 and max(int(4 * sy + 0.5), int(4 * sx + 0.5)) < 16:
            assert np.abs(got - ref).max() <= 2.5e-7 * scale  # (small stencils keep the exact arithmetic by default)


@pytest.mark.parametrize("n,sigma", [(700, 8.0), (600, 32.0), (300, 48.0)])
def test_gauss_blocked_sums_at_large_radii(gpu_ctx, n, sigma):
    """The blocked mode where it is the default -- 65, 257 and 385 taps, the widths the stencil's timings are quoted on --
    against scipy's float64 sums: <= 1e-6 of the largest value (measured 1-2e-7), on white noise (the hardest input: no
    cancellation helps) and on a smooth field with a large offset."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:n, 0:n]
    for a in (rng.standard_normal((n, n)), 40.0 + np.sin(x / 37.0) * np.cos(y / 23.0) + 0.1 * rng.standard_normal((n, n))):
        a = a.astype(np.float32)
        ref = scipy.ndimage.gaussian_filter(a, sigma=sigma)
        got = _smooth(gpu_ctx, a, sigma, sigma)
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        assert err <= 1.0e-6, err


def test_gauss_preserves_constant_and_mass(gpu_ctx):
    a = np.full((200, 130), 3.25, np.float32)
    assert np.allclose(_smooth(gpu_ctx, a, 5.0, 2.0), 3.25, rtol=1e-6)
    # reflect boundary conserves the sum
    rng = np.random.default_rng(2)
    b = rng.random((256, 256)).astype(np.float32)
    assert abs(_smooth(gpu_ctx, b, 3.0, 3.0).astype(np.float64).sum() - b.astype(np.float64).sum()) < 1e-3 * b.sum()


@pytest.mark.parametrize("weighted", [False, True])
def test_map_smooth_matches_reference(gpu_ctx, weighted):
    """ProjectionMap.smooth, map/projection.py:485-504."""
    import torch

    from maria_amd._lib import ptr
    from oracle import hotpath

    rng = np.random.default_rng(4)
    ny, nx = 180, 250
    data = rng.standard_normal((ny, nx)).astype(np.float32)
    weight = None
    if weighted:
        weight = rng.random((ny, nx)).astype(np.float32)
        weight[40:60, 100:140] = 0.0  # a hole larger than the kernel: denom == 0 -> 0
    ref, ref_denom = hotpath.map_smooth(data, weight, 2.0, 3.5)
    dev = "cuda:0"
    d_data = torch.as_tensor(data).to(dev)
    d_w = torch.as_tensor(weight).to(dev) if weighted else None
    d_out = torch.empty_like(d_data)
    d_den = torch.empty_like(d_data)
    d_tmp = torch.empty(2 * ny * nx, dtype=torch.float32, device=dev)
    gpu_ctx.call("mrx_map_smooth", ptr(d_data), ptr(d_w), ptr(d_out), ptr(d_den), ptr(d_tmp), ny, nx, 2.0, 3.5)
    got = d_out.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.abs(d_den.cpu().numpy() - ref_denom).max() <= 1e-6
    if weighted:
        assert (got[49:51, 115:125] == 0).all() and (ref[49:51, 115:125] == 0).all()


def test_philox_normals_are_standard(gpu_ctx):
    import torch

    from maria_amd._lib import ptr

    n = 1 << 20
    out = torch.empty(n, dtype=torch.float32, device="cuda:0")
    gpu_ctx.call("mrx_philox_normal", 20260612, 3, n, ptr(out))
    x = out.cpu().numpy().astype(np.float64)
    assert abs(x.mean()) < 5 / np.sqrt(n)
    assert abs(x.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs(scipy.stats.skew(x)) < 0.02 and abs(scipy.stats.kurtosis(x)) < 0.04
    assert scipy.stats.kstest(x[:100000], "norm").pvalue > 1e-4
    # another stream is another sequence; the same stream repeats exactly
    out2 = torch.empty_like(out)
    gpu_ctx.call("mrx_philox_normal", 20260612, 3, n, ptr(out2))
    assert torch.equal(out, out2)
    gpu_ctx.call("mrx_philox_normal", 20260612, 4, n, ptr(out2))
    assert abs(np.corrcoef(x, out2.cpu().numpy())[0, 1]) < 0.01


def _generate(ctx, seed, stream, ny, nx, dy, dx, r0, nu):
    import torch

    from maria_amd._lib import ptr

    out = torch.empty((ny, nx), dtype=torch.float32, device="cuda:0")
    work = torch.empty(((ny + 16) * (nx // 2 + 1), 2), dtype=torch.float32, device="cuda:0")
    ctx.call("mrx_screen_generate", seed, stream, ny, nx, dy, dx, r0, nu, ptr(out), ptr(work))
    return out.cpu().numpy()


@pytest.mark.parametrize("ny,nx", [(64, 128), (128, 64), (256, 256)])
def test_screen_fft_matches_numpy_irfft(gpu_ctx, ny, nx):
    """The hand-written LDS transforms (column FFT, half-spectrum fold, batched row FFT): a
    screen is determined by its Philox half spectrum, so rebuild that spectrum on the host from
    the library's own Philox routine and run numpy's irfft2 over it."""
    from maria_amd._lib import philox4x32
    from oracle import screens

    dy, dx, r0, nu = 5.0, 7.0, 300.0, 5.0 / 6.0
    seed, stream = 99, 2
    got = _generate(gpu_ctx, seed, stream, ny, nx, dy, dx, r0, nu)
    ref = screens.hermitian_philox_screen(philox4x32, seed, stream, ny, nx, dy, dx, r0, nu)
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()


def _generate_batch(ctx, seed, ny, nx, specs):
    """specs: list of dicts (stream, out_ny, out_nx, dy, dx, r0, nu, sigma_y, sigma_x)."""
    import ctypes as C

    import torch

    from maria_amd import _lib
    from maria_amd._lib import ptr

    outs = [torch.full((sp.get("out_ny") or ny, sp.get("out_nx") or nx), float("nan"), dtype=torch.float32, device="cuda:0") for sp in specs]
    descs = (_lib.MrxScreenDesc * len(specs))()
    for d, sp, o in zip(descs, specs, outs):
        d.d_out, d.stream = o.data_ptr(), sp["stream"]
        d.out_ny, d.out_nx, d.ld_out = sp.get("out_ny", 0), sp.get("out_nx", 0), 0
        d.dy, d.dx, d.r0, d.nu = sp["dy"], sp["dx"], sp["r0"], sp["nu"]
        d.sigma_y, d.sigma_x = sp.get("sigma_y", 0.0), sp.get("sigma_x", 0.0)
        d.d_amp = sp["amp"].data_ptr() if sp.get("amp") is not None else None
        d.periodic_beam = int(sp.get("periodic_beam", 0))
    n = C.c_size_t()
    _lib.load().mrx_screen_work_floats(ny, nx, len(specs), C.byref(n))
    work = torch.empty(n.value, dtype=torch.float32, device="cuda:0")
    ctx.call("mrx_screen_generate_batch", seed, ny, nx, descs, len(specs), ptr(work), work.numel())
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("ny,nx", [(256, 512), (2048, 2048), (64, 4096), (8192, 64)])
def test_screen_batch_with_fused_smoothing(gpu_ctx, ny, nx):
    """The batched generator with the beam smoothing folded into the FFT passes equals the
    plain generator followed by scipy.ndimage.gaussian_filter on the written block
    (atmosphere/atmosphere.py:341-344), for whole-domain and cropped screens, per-axis sigmas,
    a skipped axis and a radius beyond the fused tap table."""
    base = dict(dy=5.0, dx=6.0, r0=800.0, nu=5.0 / 6.0)
    specs = [
        dict(base, stream=0, sigma_y=4.25, sigma_x=3.5),
        dict(base, stream=1, sigma_y=0.0, sigma_x=2.0, r0=500.0),
        dict(base, stream=2, sigma_y=1.7, sigma_x=0.0, nu=1.0 / 3.0),
        dict(base, stream=3, sigma_y=2.0, sigma_x=6.0, out_ny=ny - 37, out_nx=nx - 21),
        dict(base, stream=4, sigma_y=3.0, sigma_x=3.0, out_ny=min(ny, 70), out_nx=min(nx, 50)),
        dict(base, stream=5),
    ]
    if ny * nx <= 1 << 20:
        specs.append(dict(base, stream=6, sigma_y=40.0, sigma_x=1.0))  # radius 160 > 128: separate stencil
    got = _generate_batch(gpu_ctx, 11, ny, nx, specs)
    for sp, g in zip(specs, got):
        plain = _generate(gpu_ctx, 11, sp["stream"], ny, nx, sp["dy"], sp["dx"], sp["r0"], sp["nu"])
        block = plain[: sp.get("out_ny") or ny, : sp.get("out_nx") or nx]
        ref = scipy.ndimage.gaussian_filter(block, sigma=(sp.get("sigma_y", 0.0), sp.get("sigma_x", 0.0)))
        assert g.shape == ref.shape and not np.isnan(g).any()
        assert np.abs(g - ref).max() <= 1e-5 * np.abs(ref).max(), sp


@pytest.mark.parametrize("ny,nx", [(256, 512), (2048, 2048), (1024, 4096), (64, 128)])
def test_beam_folded_into_the_spectrum_equals_the_stencil_inside(gpu_ctx, ny, nx):
    """mrx_screen_desc.periodic_beam: scipy's truncated, normalised Gaussian taps as a factor of the spectrum (their
    transfer function on the periodic domain) instead of two stencils on the written block.  Pixels at least the
    stencil radius from every edge of the block equal scipy.ndimage.gaussian_filter of the unsmoothed screen
    (atmosphere/atmosphere.py:341-344) to 1e-5 of its peak -- whole-domain and cropped blocks, per-axis sigmas, a
    skipped axis, a radius beyond the fused tap table --; on the whole domain every pixel equals the filter with
    mode="wrap"; the Stockham and the register column transforms agree."""
    from maria_amd import _lib

    base = dict(dy=5.0, dx=6.0, r0=800.0, nu=5.0 / 6.0, periodic_beam=1)
    specs = [
        dict(base, stream=0, sigma_y=4.25, sigma_x=3.5),
        dict(base, stream=1, sigma_y=0.0, sigma_x=2.0, r0=500.0),
        dict(base, stream=2, sigma_y=1.7, sigma_x=0.0, nu=1.0 / 3.0),
        dict(base, stream=3, sigma_y=2.0, sigma_x=3.0, out_ny=ny - 27, out_nx=nx - 21),
        dict(base, stream=5),
    ]
    if ny >= 1024:
        specs.append(dict(base, stream=6, sigma_y=40.0, sigma_x=1.0))  # radius 160: no tap-table limit in this form
    got = _generate_batch(gpu_ctx, 11, ny, nx, specs)
    for sp, g in zip(specs, got):
        plain = _generate(gpu_ctx, 11, sp["stream"], ny, nx, sp["dy"], sp["dx"], sp["r0"], sp["nu"])
        sig = (sp.get("sigma_y", 0.0), sp.get("sigma_x", 0.0))
        wrap = scipy.ndimage.gaussian_filter(plain, sigma=sig, mode="wrap")
        oy, ox = sp.get("out_ny") or ny, sp.get("out_nx") or nx
        assert g.shape == (oy, ox) and not np.isnan(g).any()
        assert np.abs(g - wrap[:oy, :ox]).max() <= 1e-5 * np.abs(wrap).max(), sp
        ry, rx = (int(4.0 * s_ + 0.5) if s_ > 1e-15 else 0 for s_ in sig)
        ref = scipy.ndimage.gaussian_filter(plain[:oy, :ox], sigma=sig)  # reflect at the block's edges
        inner = (slice(ry, oy - ry), slice(rx, ox - rx))
        assert np.abs(g[inner] - ref[inner]).max() <= 1e-5 * np.abs(ref).max(), sp
        if ry or rx:  # ... and the edges do differ (the two semantics are not the same thing)
            assert np.abs(g - ref).max() > 1e-4 * np.abs(ref).max()
    if ny in (1024, 2048):
        gpu_ctx.set_option(_lib.OPT_SCREEN_STOCKHAM, 1)
        try:
            other = _generate_batch(gpu_ctx, 11, ny, nx, specs[:2])
        finally:
            gpu_ctx.set_option(_lib.OPT_SCREEN_STOCKHAM, 0)
        for a, b in zip(got, other):
            assert np.abs(a - b).max() <= 2e-5 * np.abs(b).max()


def test_tap_cache_eviction_spares_the_batch_under_assembly(gpu_ctx):
    """The fused stencils' Gaussian taps are cached per (sigma, radius) in the context.  A batch whose
    first layers HIT cached slots and whose later layers MISS must not have the hit slots evicted
    before its single launch: fill and wrap the cache with 140 distinct sigmas, then
    run a batch that mixes the oldest cached sigmas with new ones and compare every layer with the
    same layer generated on its own.  (gpu_ctx only for its device set-up and its skip without a GPU.)"""
    from maria_amd import Context

    ctx = Context(0)  # a cache of its own
    ny = nx = 128
    base = dict(dy=5.0, dx=5.0, r0=300.0, nu=5.0 / 6.0)
    sig = lambda k: 0.8 + 0.01 * k  # noqa: E731
    for k0 in range(0, 140, 14):  # 140 distinct sigma_y (radius 3-9): the 128 slots wrap
        _generate_batch(ctx, 3, ny, nx, [dict(base, stream=k, sigma_y=sig(k), sigma_x=0.0) for k in range(k0, k0 + 14)])
    # now cached: sigmas 12 .. 139 (0 .. 11 were evicted).  The batch: 8 hits on the OLDEST cached slots -- the
    # next to be evicted -- followed by 8 misses
    specs = [dict(base, stream=100 + i, sigma_y=sig(12 + i), sigma_x=0.0) for i in range(8)]
    specs += [dict(base, stream=200 + i, sigma_y=2.5 + 0.013 * i, sigma_x=0.0) for i in range(8)]
    got = _generate_batch(ctx, 3, ny, nx, specs)
    fresh = Context(0)
    for sp, g in zip(specs, got):
        alone = _generate_batch(fresh, 3, ny, nx, [sp])[0]
        assert np.array_equal(g, alone), sp


@pytest.mark.parametrize("ny,nx", [(1024, 512), (2048, 2048), (4096, 256), (2048, 1024), (256, 4096), (128, 8192), (1024, 4096)])
def test_register_transforms_match_the_stockham_ones(gpu_ctx, ny, nx):
    """Sides of 1024, 2048 and 4096 take the transforms in registers (fft_regs: 16 x RB x 16, the
    spectrum cells drawn straight into the first pass's registers); MRX_OPT_SCREEN_STOCKHAM keeps
    the LDS Stockham kernels.  Same Philox cells: the screens agree to float32 rounding -- plain,
    smoothed, cropped -- and so do the planes of a 3-D volume (pass 1 fed from the work buffer).
    One size also against numpy's irfft2 of the same spectrum."""
    from maria_amd import _lib

    base = dict(dy=5.0, dx=6.0, r0=800.0, nu=5.0 / 6.0)
    specs = [dict(base, stream=0), dict(base, stream=1, sigma_y=4.25, sigma_x=3.5),
             dict(base, stream=2, sigma_y=2.0, sigma_x=6.0, out_ny=ny - 37, out_nx=nx - 21)]
    got = _generate_batch(gpu_ctx, 17, ny, nx, specs)
    gpu_ctx.set_option(_lib.OPT_SCREEN_STOCKHAM, 1)
    try:
        ref = _generate_batch(gpu_ctx, 17, ny, nx, specs)
    finally:
        gpu_ctx.set_option(_lib.OPT_SCREEN_STOCKHAM, 0)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.abs(r).max() > 1 and np.abs(g - r).max() <= 3e-6 * np.abs(r).max()
    if (ny, nx) == (1024, 512):
        from maria_amd._lib import philox4x32
        from oracle import screens

        want = screens.hermitian_philox_screen(philox4x32, 17, 0, ny, nx, 5.0, 6.0, 800.0, 5.0 / 6.0)
        assert np.abs(got[0] - want).max() <= 2e-5 * np.abs(want).max()
        args = (8, ny, nx, 30.0, 20.0, 25.0, 400.0, 1.0 / 3.0)
        vol = _generate_3d(gpu_ctx, 5, 3, *args, [0.0, 2.5, 6.75], [1.0, 1.1, 0.9], sigma=2.0)
        gpu_ctx.set_option(_lib.OPT_SCREEN_STOCKHAM, 1)
        try:
            vol_ref = _generate_3d(gpu_ctx, 5, 3, *args, [0.0, 2.5, 6.75], [1.0, 1.1, 0.9], sigma=2.0)
        finally:
            gpu_ctx.set_option(_lib.OPT_SCREEN_STOCKHAM, 0)
        for g, r in zip(vol, vol_ref):
            assert np.abs(g - r).max() <= 3e-6 * np.abs(r).max()


def test_screen_statistics_match_matern(gpu_ctx):
    """Generator parity is statistical.  Two steps, so that the tolerance on the
    device code is the sampling noise alone:
    (1) the screens against the generator's own target, the covariance of a periodic field with
        the discrete spectrum amp^2 (its inverse transform, exact): unit variance within 4 sigma of
        its own sampling noise (the largest modes carry it) and the structure function at eight lags
        on both axes to 4 %, over 48 independent 1024^2 screens;
    (2) that target against Matern(nu = 5/6, r0) of functions/__init__.py:30-74 (numpy only): the
        periodic 5.1 km box removes the power below 1/L and the grid aliases the rest -- the
        structure function stays within 10 % of Matern's up to 128 pixels."""
    from oracle import functions, screens

    ny = nx = 1024
    d, r0, nu = 5.0, 1000.0, 5.0 / 6.0
    lags = np.array([0, 1, 2, 4, 8, 16, 32, 64, 128])
    acc = np.zeros((2, len(lags)))
    nrep = 48
    for rep in range(nrep):
        s = _generate(gpu_ctx, 20260612, rep, ny, nx, d, d, r0, nu)
        (r, cy), (_, cx) = screens.radial_covariance(s, d, d, lags)
        acc += np.array([cy, cx]) / nrep
    power = screens.psd_amplitude(ny, nx, d, d, r0, nu) ** 2
    model = np.fft.ifft2(power).real
    model /= model[0, 0]
    # the variance of one screen is carried by its few largest modes: its sampling noise follows
    # from the spectrum, std = sqrt(2 sum P^2) / sum P -- 0.41 a screen at r0 = 1 km in a 5 km box
    var_tol = 4.0 * np.sqrt(2.0 * (power**2).sum()) / power.sum() / np.sqrt(nrep)
    # so the unit variance is checked where it can be: r0 = 30 m has thousands of independent patches a
    # screen (4 sigma of the mean of 48 screens of 512^2: 1.4 %)
    small = [np.mean(_generate(gpu_ctx, 7, rep, 512, 512, d, d, 30.0, nu).astype(np.float64) ** 2) for rep in range(48)]
    p30 = screens.psd_amplitude(512, 512, d, d, 30.0, nu) ** 2
    tol30 = 4.0 * np.sqrt(2.0 * (p30**2).sum()) / p30.sum() / np.sqrt(48)
    assert tol30 < 0.02 and abs(np.mean(small) - 1) < tol30, (np.mean(small), tol30)
    want = np.array([model[lags, 0], model[0, lags]])
    sf_got = 2 * (acc[:, :1] - acc[:, 1:])
    sf_want = 2 * (want[:, :1] - want[:, 1:])
    assert np.abs(acc[:, 0] - 1).max() < var_tol, (acc[:, 0], var_tol)
    assert np.abs(sf_got / sf_want - 1).max() < 0.04, (sf_got, sf_want)
    target = functions.approximate_normalized_matern(lags * d, nu=nu, r0=r0)
    sf_ref = 2 * (target[0] - target[1:])
    assert np.abs(sf_want / sf_ref[None] - 1).max() < 0.10, (sf_want, sf_ref)


def test_screen_is_reproducible_and_layer_independent(gpu_ctx):
    # outer scale well inside the 1.3 km box, so that a screen holds many independent modes
    a = _generate(gpu_ctx, 7, 0, 256, 256, 5.0, 5.0, 100.0, 5.0 / 6.0)
    b = _generate(gpu_ctx, 7, 0, 256, 256, 5.0, 5.0, 100.0, 5.0 / 6.0)
    c = _generate(gpu_ctx, 7, 1, 256, 256, 5.0, 5.0, 100.0, 5.0 / 6.0)  # another stream: another draw
    assert np.array_equal(a, b)
    assert abs(np.corrcoef(a.ravel(), c.ravel())[0, 1]) < 0.1
    assert not np.isnan(a).any()


def test_generate_screens_end_to_end(gpu_ctx):
    """Screens made on the device feed the sampling kernel; the oracle, given the
    same (downloaded) screens, agrees to 1e-5."""
    from maria_amd import synthetic
    from maria_amd.pipeline import DevicePath
    from oracle import hotpath

    p = synthetic.make_problem(n_det=100, n_bands=2, fov_deg=0.5, fs=100.0, duration=30.0, n_layers=4, side=256)
    path = DevicePath(p, device="cuda:0", ctx=gpu_ctx)
    scr = path.generate_screens()
    tod = path.run().cpu().numpy()
    assert path.check_flags() == 0
    for layer, s in zip(p["layers"], scr):
        layer["values"] = s.cpu().numpy()
    ref = hotpath.run_path(p)
    assert rel_err(tod, ref) <= 1e-5


@pytest.mark.parametrize("n,lj", [(4, 0), (8, 0), (64, 0), (128, 0), (2048, 0), (4096, 0), (8192, 0), (64, 6), (128, 5), (1024, 2), (4, 3), (32, 4), (64, -1), (4096, -2), (1024, -3), (2048, -3), (4096, -3)])
def test_lds_fft_matches_numpy(gpu_ctx, n, lj):
    """The in-LDS Stockham transform (and its interleaved-sequences form) against
    numpy.fft.ifft: the building block of both spectral generators."""
    import torch

    from maria_amd._lib import ptr

    rng = np.random.default_rng(n + lj)
    # lj = -1: the 64-point register transform; lj = -2: the 4096-point radix-16 workgroup transform;
    # lj = -3: fft_regs<RB> (16 x RB x 16, RB = 4, 8, 16: several rows per workgroup, an odd row count)
    rows, J = (3, 1 << lj) if lj >= 0 else (200 if lj == -1 else 5, 1)
    x = (rng.normal(size=(rows, n, J)) + 1j * rng.normal(size=(rows, n, J))).astype(np.complex64)
    d_in = torch.as_tensor(np.ascontiguousarray(x)).to("cuda:0")
    d_out = torch.empty_like(d_in)
    gpu_ctx.call("mrx_fft_rows", ptr(d_in), rows, n, lj, ptr(d_out))
    got = d_out.cpu().numpy()
    ref = np.fft.ifft(x.astype(np.complex128), axis=1) * n
    assert np.abs(got - ref).max() <= 1e-6 * np.log2(n) * np.abs(ref).max()


def _generate_3d(ctx, seed, stream, nh, ny, nx, dh, dy, dx, r0, nu, plane_pos, plane_scale=None, sigma=0.0, out_shape=None, amp=None):
    import ctypes as C

    import torch

    from maria_amd import _lib
    from maria_amd._lib import ptr

    n = len(plane_pos)
    oy, ox = out_shape or (ny, nx)
    outs = [torch.full((oy, ox), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(n)]
    descs = (_lib.MrxScreenDesc * n)()
    for d, o in zip(descs, outs):
        d.d_out, d.out_ny, d.out_nx, d.ld_out = o.data_ptr(), oy, ox, 0
        d.sigma_y = d.sigma_x = sigma
    need = C.c_size_t()
    _lib.load().mrx_screen3d_work_floats(nh, ny, nx, n, C.byref(need))
    work = torch.empty(need.value, dtype=torch.float32, device="cuda:0")
    pos = (C.c_double * n)(*plane_pos)
    scl = (C.c_double * n)(*plane_scale) if plane_scale is not None else None
    ctx.call("mrx_screen_generate_3d", seed, stream, nh, ny, nx, dh, dy, dx, r0, nu, pos, scl, descs, n, ptr(work), work.numel(), ptr(amp))
    return [o.cpu().numpy() for o in outs]


def test_screen_3d_matches_numpy(gpu_ctx):
    """The three transform passes of the 3-D generator against numpy on the same Philox cells:
    on-grid and interpolated planes, with a variance scale."""
    from maria_amd._lib import philox4x32
    from oracle import screens

    nh, ny, nx = 8, 64, 64
    args = (nh, ny, nx, 30.0, 20.0, 25.0, 400.0, 1.0 / 3.0)
    pos, scale = [0.0, 2.5, 6.0, 6.75], [1.0, 1.1, 1.0, 0.9]
    got = _generate_3d(gpu_ctx, 5, 3, *args, pos, scale)
    ref = screens.hermitian_philox_screens_3d(philox4x32, 5, 3, *args, pos, scale)
    for g, r in zip(got, ref):
        assert np.abs(g - r).max() <= 3e-5 * np.abs(r).max()


def test_screen_3d_statistics_match_matern(gpu_ctx):
    """model="3d": layers of one process are slices of a 3-D Matern(nu = 1/3, r0) field
    (atmosphere/atmosphere.py:249): unit variance, the Matern structure function inside a
    plane, and the same function of the vertical separation between planes."""
    from oracle import functions, screens

    nh, ny, nx = 256, 256, 256
    d, r0, nu = 20.0, 600.0, 1.0 / 3.0
    pos = [40.0, 41.0, 42.0, 44.0, 48.0, 56.0, 72.0]
    lags = np.array([1, 2, 4, 8, 16, 32])
    var, sf_v, sf_x = [], np.zeros(len(pos) - 1), np.zeros(len(lags))
    nrep = 6
    for rep in range(nrep):
        planes = _generate_3d(gpu_ctx, 77, rep, nh, ny, nx, d, d, d, r0, nu, pos)
        base = planes[0].astype(np.float64)
        var.append(np.mean([np.mean(p.astype(np.float64) ** 2) for p in planes]))
        # structure functions directly (differences: the large-scale modes of a realisation cancel)
        sf_v += np.array([np.mean((base - p) ** 2) for p in planes[1:]]) / nrep
        sf_x += np.array([np.mean((base - np.roll(base, -k, axis=1)) ** 2) for k in lags]) / nrep
    assert abs(np.mean(var) - 1) < 0.08, var
    dz = (np.array(pos[1:]) - pos[0]) * d
    # (1) the generator's own definition: covariance = inverse transform of the squared amplitudes
    amp2 = screens.psd_amplitude_3d(nh, ny, nx, d, d, d, r0, nu) ** 2
    model = np.fft.ifftn(amp2).real
    model /= model[0, 0, 0]
    want_v = 2 * (1 - model[(np.array(pos[1:]) - pos[0]).astype(int), 0, 0])
    want_x = 2 * (1 - model[0, 0, lags])
    assert np.abs(sf_v / want_v - 1).max() < 0.1, (sf_v, want_v)
    assert np.abs(sf_x / want_x - 1).max() < 0.1, (sf_x, want_x)
    # (2) the target, Matern(nu = 1/3): the spectrum stops at the grid's Nyquist frequency, which
    # matters for so rough a field (structure function ~ r^(2/3)) only within a few pixels -- the
    # scales the beam smoothing removes anyway (3d layers: sigma >= 0.85 pixel, extrusion.py:20-22)
    ref = lambda r: functions.approximate_normalized_matern(np.asarray(r, float), nu=nu, r0=r0)  # noqa: E731
    far_v, far_x = dz >= 8 * d, lags >= 8
    assert np.abs(sf_v[far_v] / (2 * (1 - ref(dz[far_v]))) - 1).max() < 0.15, (sf_v, 2 * (1 - ref(dz)))
    assert np.abs(sf_x[far_x] / (2 * (1 - ref(lags[far_x] * d))) - 1).max() < 0.15, (sf_x, 2 * (1 - ref(lags * d)))
    # deterministic, and another stream is another field
    a = _generate_3d(gpu_ctx, 77, 0, nh, ny, nx, d, d, d, r0, nu, pos[:2])
    b = _generate_3d(gpu_ctx, 77, 0, nh, ny, nx, d, d, d, r0, nu, pos[:2])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_resample_columns_matches_numpy(gpu_ctx):
    """mrx_resample_columns (model="3d": a layer's own cross-section nodes from the generation grid): the scaled
    linear blend of the two bracketing columns, rows with a pitch, first and last columns, and its argument checks."""
    import torch

    from maria_amd import MrxError
    from maria_amd._lib import ptr

    rng = np.random.default_rng(8)
    n_e, n_in, ld_in, n_out, ld_out = 300, 41, 45, 29, 33
    src = rng.standard_normal((n_e, ld_in)).astype(np.float32)
    u = np.sort(rng.uniform(0, n_in - 1, n_out))
    u[0], u[-1] = 0.0, n_in - 1.0
    idx = np.clip(np.floor(u).astype(np.int32), 0, n_in - 2)
    w = (u - idx).astype(np.float32)
    scale = rng.uniform(1.0, 1.05, n_out).astype(np.float32)
    want = scale * ((1 - w) * src[:, idx] + w * src[:, idx + 1])
    dev = "cuda:0"
    d_src, d_idx, d_w, d_s = (torch.as_tensor(a).to(dev) for a in (src, idx, w, scale))
    d_out = torch.full((n_e, ld_out), -3.0, dtype=torch.float32, device=dev)
    gpu_ctx.call("mrx_resample_columns", ptr(d_src), n_e, n_in, ld_in, ptr(d_idx), ptr(d_w), ptr(d_s), n_out, ptr(d_out), ld_out)
    got = d_out.cpu().numpy()
    assert (got[:, n_out:] == -3.0).all()
    assert np.abs(got[:, :n_out] - want).max() <= 3e-7 * np.abs(want).max()
    with pytest.raises(MrxError, match="INVALID"):
        gpu_ctx.call("mrx_resample_columns", ptr(d_src), n_e, n_in, ld_in, ptr(d_idx), ptr(d_w), ptr(d_s), n_out, ptr(d_out), n_out - 1)
    gpu_ctx.call("mrx_resample_columns", ptr(d_src), 0, n_in, ld_in, ptr(d_idx), ptr(d_w), ptr(d_s), n_out, ptr(d_out), ld_out)  # empty: no-op


# ---- covariance-matched amplitudes (mrx_screen_amplitudes) --------------------------------


def _amp_table(ctx, nh, ny, nx, dh, dy, dx, r0, nu):
    import ctypes as C

    import torch

    from maria_amd import _lib
    from maria_amd._lib import ptr
    from maria_amd.pipeline import matern_log_tables

    log_first, log_step, log_cov, log_sf, x_cut = matern_log_tables(nu)
    n_t, n_w = C.c_size_t(), C.c_size_t()
    _lib.load().mrx_screen_amp_floats(nh, ny, nx, len(log_cov), C.byref(n_t), C.byref(n_w))
    table = torch.empty(n_t.value, dtype=torch.float32, device="cuda:0")
    work = torch.empty(n_w.value, dtype=torch.float32, device="cuda:0")
    as_d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ctx.call("mrx_screen_amplitudes", nh, ny, nx, dh, dy, dx, r0, as_d(log_cov), as_d(log_sf), len(log_cov), log_first, log_step,
             x_cut, ptr(table), ptr(work), work.numel())
    return table


def _unfold(table, nh, ny, nx):
    """The device table [kx][kz][ky] over the half axes -> (sum, full [nh or 1, ny, nx] amplitudes)."""
    host = table.cpu().numpy()
    mz, my, mx = (nh // 2 + 1 if nh else 1), ny // 2 + 1, nx // 2 + 1
    total = float(host[:2].view(np.float64)[0])
    half = host[4 : 4 + mx * mz * my].reshape(mx, mz, my).transpose(1, 2, 0)  # [kz][ky][kx]
    fold = lambda n: np.minimum(np.arange(n), n - np.arange(n))  # noqa: E731
    full = half[np.ix_(fold(nh) if nh else np.zeros(1, int), fold(ny), fold(nx))]
    return total, full


@pytest.mark.parametrize("nh,ny,nx,nu,r0", [(0, 128, 64, 5 / 6, 300.0), (0, 256, 1024, 5 / 6, 300.0), (0, 2048, 64, 1 / 3, 100.0),
                                            (0, 8192, 64, 5 / 6, 150.0),  # the longest axis: 98 KB of LDS for its cosine sums
                                            (8, 64, 128, 1 / 3, 40.0), (32, 128, 64, 1 / 3, 60.0)])
def test_amplitude_table_matches_numpy_fft(gpu_ctx, nh, ny, nx, nu, r0):
    """The table of mrx_screen_amplitudes (periodic images summed, float64 cosine sums over the even half
    axes, the radial correlation by Lagrange interpolation of the host's log-log table) against numpy's FFT
    of scipy's exact Matern correlation summed over the same images; the header normalises the screens to
    Matern's structure function.  Boxes of 1 ... 30 outer scales a side: up to 59 images per axis."""
    from maria_amd.pipeline import matern_log_tables
    from oracle import functions, screens

    dh, dy, dx = 40.0, 5.0, 7.0
    table = _amp_table(gpu_ctx, nh, ny, nx, dh, dy, dx, r0, nu)
    total, got = _unfold(table, nh, ny, nx)
    shape, steps = ((nh, ny, nx), (dh, dy, dx)) if nh else ((ny, nx), (dy, dx))
    ref, rho0 = screens.covariance_amplitude(shape, steps, r0, nu, x_cut=matern_log_tables(nu)[4])
    ref = ref.reshape(got.shape)
    assert np.abs(got - ref).max() <= 2e-6 * ref.max()
    big = ref > 1e-3 * ref.max()
    assert np.abs(got[big] / ref[big] - 1).max() <= 1e-5
    assert abs(total / ((ref.astype(np.float32).astype(np.float64) ** 2).sum() / rho0) - 1) <= 1e-6
    # positive definite: next to nothing is clipped
    assert (got == 0).mean() < 1e-3
    # what the table is for: the structure function of the field it defines, from one pixel up
    cov = np.fft.ifftn(got.astype(np.float64) ** 2).real.reshape(-1) * got.size / total
    lags = np.array([1, 2, 5])
    want = functions.normalized_matern(lags * dx / r0, nu)
    # (the images' curvature enters at second order in lag / period: 4e-3 in a box of 4.5 outer scales, 10 % in the
    # first case's 1.5)
    assert np.abs((cov[0] - cov[lags]) / (1 - want) - 1).max() < (5e-3 if min(ny * dy, nx * dx) > 4 * r0 else 0.15)


@pytest.mark.parametrize("ny,nx", [(64, 128), (1024, 64), (2048, 64)])
def test_screen_with_amplitude_table_matches_numpy_irfft(gpu_ctx, ny, nx):
    """Both column forms (LDS and register transforms) read the table for the cells they draw: the screen
    equals numpy's irfft2 of the same Philox cells times the oracle's amplitudes."""
    from maria_amd._lib import philox4x32
    from oracle import screens

    dy, dx, r0, nu = 5.0, 7.0, 300.0, 5.0 / 6.0
    seed, stream = 99, 2
    table = _amp_table(gpu_ctx, 0, ny, nx, 0.0, dy, dx, r0, nu)
    got = _generate_batch(gpu_ctx, seed, ny, nx, [dict(stream=stream, dy=dy, dx=dx, r0=r0, nu=nu, amp=table)])[0]
    from maria_amd.pipeline import matern_log_tables

    amp, rho0 = screens.covariance_amplitude((ny, nx), (dy, dx), r0, nu, x_cut=matern_log_tables(nu)[4])
    ref = screens.hermitian_philox_screen(philox4x32, seed, stream, ny, nx, dy, dx, r0, nu, amp=amp) * np.sqrt(rho0)
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()


def test_screen_3d_with_amplitude_table_matches_numpy(gpu_ctx):
    from maria_amd._lib import philox4x32
    from oracle import screens

    nh, ny, nx = 8, 64, 64
    args = (nh, ny, nx, 30.0, 20.0, 25.0, 400.0, 1.0 / 3.0)
    pos, scale = [0.0, 2.5, 6.0, 6.75], [1.0, 1.1, 1.0, 0.9]
    table = _amp_table(gpu_ctx, *args)
    got = _generate_3d(gpu_ctx, 5, 3, *args, pos, scale, amp=table)
    from maria_amd.pipeline import matern_log_tables

    amp, rho0 = screens.covariance_amplitude((nh, ny, nx), (30.0, 20.0, 25.0), 400.0, 1.0 / 3.0, x_cut=matern_log_tables(1.0 / 3.0)[4])
    ref = screens.hermitian_philox_screens_3d(philox4x32, 5, 3, *args, pos, scale, amp=amp)
    for g, r in zip(got, ref):
        assert np.abs(g - np.sqrt(rho0) * r).max() <= 3e-5 * np.abs(r).max()


def test_screen_statistics_with_amplitude_table_are_matern(gpu_ctx):
    """With the covariance-matched amplitudes the generator's target IS the reference's covariance
    (functions/__init__.py:42-74), so the measured structure function is held against it directly --
    from ONE pixel up, for the smooth 2-D field (nu = 5/6) and the rough 3-D one (nu = 1/3), where the
    power law is several times low at one pixel."""
    from oracle import functions, screens

    # two dimensions
    ny = nx = 1024
    d, r0, nu = 5.0, 1000.0, 5.0 / 6.0
    lags = np.array([0, 1, 2, 4, 8, 16, 32, 64, 128])
    table = _amp_table(gpu_ctx, 0, ny, nx, 0.0, d, d, r0, nu)
    acc = np.zeros((2, len(lags)))
    nrep = 48
    for rep in range(0, nrep, 16):
        specs = [dict(stream=rep + i, dy=d, dx=d, r0=r0, nu=nu, amp=table) for i in range(16)]
        for s in _generate_batch(gpu_ctx, 20260612, ny, nx, specs):
            (_, cy), (_, cx) = screens.radial_covariance(s, d, d, lags)
            acc += np.array([cy, cx]) / nrep
    sf_got = 2 * (acc[:, :1] - acc[:, 1:])
    target = functions.approximate_normalized_matern(lags * d, nu=nu, r0=r0)
    sf_ref = 2 * (target[0] - target[1:])
    assert np.abs(sf_got / sf_ref[None] - 1).max() < 0.05, (sf_got, sf_ref)
    assert np.abs(sf_got[:, :3] / sf_ref[None, :3] - 1).max() < 0.01, (sf_got, sf_ref)  # 1, 2, 4 pixels: little sampling noise

    # three dimensions, nu = 1/3
    nh, ny, nx = 256, 256, 256
    d, r0, nu = 20.0, 600.0, 1.0 / 3.0
    pos = [40.0, 41.0, 42.0, 44.0, 48.0, 56.0, 72.0]
    lags = np.array([1, 2, 4, 8, 16, 32])
    table = _amp_table(gpu_ctx, nh, ny, nx, d, d, d, r0, nu)
    var, sf_v, sf_x = [], np.zeros(len(pos) - 1), np.zeros(len(lags))
    nrep = 6
    for rep in range(nrep):
        planes = _generate_3d(gpu_ctx, 77, rep, nh, ny, nx, d, d, d, r0, nu, pos, amp=table)
        base = planes[0].astype(np.float64)
        var.append(np.mean([np.mean(p.astype(np.float64) ** 2) for p in planes]))
        sf_v += np.array([np.mean((base - p) ** 2) for p in planes[1:]]) / nrep
        sf_x += np.array([np.mean((base - np.roll(base, -k, axis=1)) ** 2) for k in lags]) / nrep
    assert abs(np.mean(var) - 1) < 0.08, var
    ref = lambda r: functions.normalized_matern(np.asarray(r, float) / r0, nu)  # noqa: E731
    dz = (np.array(pos[1:]) - pos[0]) * d
    # measured 0.1 % at one pixel (the power law: 4x low there), 1 % up to 16, 8 % at 32 pixels = one outer scale,
    # where six realisations of 256^2 hold few independent patches
    err_v, err_x = np.abs(sf_v / (2 * (1 - ref(dz))) - 1), np.abs(sf_x / (2 * (1 - ref(lags * d))) - 1)
    assert err_v.max() < 0.12 and err_v[dz <= 8 * d].max() < 0.03, (sf_v, 2 * (1 - ref(dz)))
    assert err_x.max() < 0.12 and err_x[lags <= 8].max() < 0.03, (sf_x, 2 * (1 - ref(lags * d)))


def test_amplitude_table_errors(gpu_ctx):
    import ctypes as C

    import torch

    from maria_amd._lib import MrxError, ptr
    from maria_amd.pipeline import matern_log_tables

    log_first, log_step, log_cov, log_sf, x_cut = matern_log_tables(5 / 6)
    as_d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    table = torch.empty(1 << 16, dtype=torch.float32, device="cuda:0")
    work = torch.empty(1 << 10, dtype=torch.float32, device="cuda:0")
    with pytest.raises(MrxError, match="work buffer"):
        gpu_ctx.call("mrx_screen_amplitudes", 0, 64, 64, 0.0, 5.0, 5.0, 300.0, as_d(log_cov), as_d(log_sf), len(log_cov), log_first,
                     log_step, x_cut, ptr(table), ptr(work), work.numel())
    with pytest.raises(MrxError, match="powers of two"):
        gpu_ctx.call("mrx_screen_amplitudes", 0, 96, 64, 0.0, 5.0, 5.0, 300.0, as_d(log_cov), as_d(log_sf), len(log_cov), log_first,
                     log_step, x_cut, ptr(table), ptr(table), table.numel())
    with pytest.raises(MrxError, match="too small against x_cut"):
        gpu_ctx.call("mrx_screen_amplitudes", 0, 64, 64, 0.0, 0.01, 0.01, 3000.0, as_d(log_cov), as_d(log_sf), len(log_cov), log_first,
                     log_step, x_cut, ptr(table), ptr(table), table.numel())
