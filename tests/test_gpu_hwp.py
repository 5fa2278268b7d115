"""mrx_tod_demodulate, mrx_tod_hwp_modulate, maria_amd.hwp, Simulation(hwp=...), TOD.demodulate and TOD.remove_hwpss on the
device, against the float64 formulas of tests/hwp_ref.py evaluated on the float32 inputs.

Tolerances of the kernel comparisons (they extend tests/test_gpu_downsample.py's): y_t within
2^-23 |ref| + 1e-12 sum|hT| max|x| / min(den), y_q and y_u within 2^-23 |ref| + 2e-12 sum|hP| max|c x| / min(den): one
float32 rounding, and slack for the order of a float64 sum of at most 1025 terms (1025 * 2^-53 = 1.1e-13)."""

import hwp_ref as ref
import numpy as np
import pytest
import scipy.signal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def noise_rows(D, T, seed=0):
    return (np.random.default_rng(seed).standard_normal((D, T)) + 5).astype(np.float32)


def random_carrier(T, seed=1):
    """Random numbers, not of unit modulus: a swapped cos / sin or a missing factor 2 shows."""
    return np.random.default_rng(seed).standard_normal((T, 2))


def two_lowpasses(n_taps, q):
    """hT != hP."""
    if n_taps == 1:
        return np.array([1.0]), np.array([0.5])
    return scipy.signal.firwin(n_taps, 1.0 / q), scipy.signal.firwin(n_taps, 0.7 / q)


def run(gpu_ctx, x, c, q, ht, hp, pad_x=0, pad_y=0, want_t=True):
    """hwp.demodulate() of the [D, T] float32 array x held at row pitch T + pad_x, into rows of pitch T_out + pad_y of
    three buffers pre-filled with 7.0; asserts that nothing but the outputs was written and that the input is bit-identical
    after.  (y_t, y_q, y_u) as numpy arrays, y_t None without want_t."""
    import torch

    from maria_amd import downsample, hwp

    D, T = x.shape
    T_out = downsample.output_length(T, q)
    ld_x, ld_y = T + pad_x, T_out + pad_y
    xbuf = torch.full((D * ld_x + 64,), -3.0, dtype=torch.float32, device=DEV)
    xv = torch.as_strided(xbuf, (D, T), (ld_x, 1))
    xv.copy_(torch.as_tensor(x))
    before = xbuf.clone()
    dc = torch.as_tensor(c).to(DEV)
    c_before = dc.clone()
    bufs = [torch.full((D * ld_y + 64,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    views = [torch.as_strided(b, (D, T_out), (ld_y, 1)) for b in bufs]
    out = hwp.demodulate(xv, dc, q, taps_t=ht, taps_p=hp, ctx=gpu_ctx, out=(views[0] if want_t else None, views[1], views[2]), want_t=want_t)
    torch.cuda.synchronize()
    assert out[1] is views[1] and out[2] is views[2] and (out[0] is views[0] if want_t else out[0] is None)
    assert torch.equal(xbuf, before) and torch.equal(dc, c_before), "an input changed"
    ys = [v.cpu().numpy() for v in views]
    for k in ((0, 1, 2) if want_t else (1, 2)):
        views[k].fill_(7.0)
    for b in bufs:
        assert bool((b == 7.0).all()), "written outside the outputs"
    return (ys[0] if want_t else None), ys[1], ys[2]


def check(gpu_ctx, x, c, q, ht, hp, **pads):
    y_t, y_q, y_u = run(gpu_ctx, x, c, q, ht, hp, **pads)
    r_t, r_q, r_u, den_t, den_p = ref.demodulate(x, c, q, ht, hp)
    x64 = x.astype(np.float64)
    worst = []
    for y, r, tol in ((y_t, r_t, ref.tolerance_t(r_t, x, ht, den_t)),
                      (y_q, r_q, ref.tolerance_p(r_q, c[None, :, 0] * x64, hp, den_p)),
                      (y_u, r_u, ref.tolerance_p(r_u, c[None, :, 1] * x64, hp, den_p))):
        assert y.shape == r.shape and y.dtype == np.float32
        worst.append(float((np.abs(y.astype(np.float64) - r) / tol).max()))
    print(f"D {x.shape[0]} T {x.shape[1]} q {q} taps {len(ht)}: max |y - ref| / tolerance = T {worst[0]:.3f} Q {worst[1]:.3f} U {worst[2]:.3f}")
    assert max(worst) <= 1.0
    return y_t, y_q, y_u


@pytest.mark.parametrize("D,T,q,n_taps,pad_x,pad_y", [
    (1, 1, 2, 1, 0, 0),            # a single sample
    (3, 37, 2, 41, 0, 0),          # T < n_taps: every output truncated on both sides, odd T
    (2, 100, 16, 321, 0, 0),       # T < H
    (5, 1000, 4, 81, 3, 1),        # padded, unaligned rows
    (130, 5000, 4, 81, 0, 0),      # many rows, a count that divides nothing
    (3, 70001, 32, 1025, 0, 0),    # the worst LDS shape
    (2, 240000, 8, 523, 0, 0),     # benchmark-length rows, many tiles
])
def test_demodulate_matches_the_formula(gpu_ctx, D, T, q, n_taps, pad_x, pad_y):
    check(gpu_ctx, noise_rows(D, T, seed=T), random_carrier(T, seed=T + 1), q, *two_lowpasses(n_taps, q), pad_x=pad_x, pad_y=pad_y)


@pytest.mark.parametrize("tiles,extra", [(1, -1), (1, 0), (1, 1), (2, 1)])
def test_tile_seams(gpu_ctx, tiles, extra):
    """T_out one short of a workgroup's run of outputs, exactly one run, one more, and two runs and one: the seam and the
    halo across it."""
    from maria_amd import downsample, hwp

    T_out = tiles * hwp.TILE_OUTPUTS + extra
    T = 8 * T_out - 3
    assert downsample.output_length(T, 8) == T_out
    check(gpu_ctx, noise_rows(4, T, seed=extra + 7), random_carrier(T, seed=tiles), 8, *two_lowpasses(161, 8))


@pytest.mark.parametrize("D,T,q,n_taps", [(2, 100, 16, 321), (5, 1000, 4, 81), (3, 70001, 32, 1025), (7, 9001, 8, 523)])
def test_the_t_series_is_the_decimators_and_runs_repeat(gpu_ctx, D, T, q, n_taps):
    """y_t equals downsample.decimate(x, q, hT) bit for bit (the same sum in the same order over the same denominators, the
    truncated edges included); without y_t, Q and U are the bits of the three-output call; two runs are bit-identical."""
    import torch

    from maria_amd import downsample

    x, c = noise_rows(D, T, seed=T + 2), random_carrier(T, seed=T + 3)
    ht, hp = two_lowpasses(n_taps, q)
    y_t, y_q, y_u = run(gpu_ctx, x, c, q, ht, hp)
    dec = downsample.decimate(torch.as_tensor(x).to(DEV), q, taps=ht, ctx=gpu_ctx).cpu().numpy()
    np.testing.assert_array_equal(y_t.view(np.uint32), dec.view(np.uint32))
    none, q_only, u_only = run(gpu_ctx, x, c, q, ht, hp, want_t=False)
    assert none is None
    np.testing.assert_array_equal(q_only.view(np.uint32), y_q.view(np.uint32))
    np.testing.assert_array_equal(u_only.view(np.uint32), y_u.view(np.uint32))
    again = run(gpu_ctx, x, c, q, ht, hp)
    for a, b in zip(again, (y_t, y_q, y_u)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_one_tap_picks_and_mixes_bit_for_bit(gpu_ctx):
    x, c = noise_rows(2, 1025, seed=3), random_carrier(1025, seed=4)
    y_t, y_q, y_u = run(gpu_ctx, x, c, 3, np.array([1.0]), np.array([1.0]))
    np.testing.assert_array_equal(y_t, x[:, ::3])
    x64 = x.astype(np.float64)
    np.testing.assert_array_equal(y_q, (2.0 * (c[None, :, 0] * x64)).astype(np.float32)[:, ::3])
    np.testing.assert_array_equal(y_u, (2.0 * (c[None, :, 1] * x64)).astype(np.float32)[:, ::3])


def test_asymmetric_taps_fix_the_orientation(gpu_ctx):
    """Random asymmetric taps (all positive: every truncated sum is): a convolution instead of the correlation fails."""
    rng = np.random.default_rng(12)
    ht = rng.uniform(0.05, 1.0, 33) * np.linspace(0.2, 2.0, 33)
    hp = rng.uniform(0.05, 1.0, 33) * np.linspace(2.0, 0.2, 33)
    x, c = noise_rows(3, 4001, seed=4), random_carrier(4001, seed=5)
    ys = check(gpu_ctx, x, c, 5, ht, hp)
    f_t, f_q, f_u, den_t, den_p = ref.demodulate(x, c, 5, ht[::-1], hp[::-1])
    x64 = x.astype(np.float64)
    assert np.abs(ys[0] - f_t).max() > 100 * ref.tolerance_t(f_t, x, ht, den_t).max()  # the test can tell the two apart
    assert np.abs(ys[1] - f_q).max() > 100 * ref.tolerance_p(f_q, c[None, :, 0] * x64, hp, den_p).max()
    assert np.abs(ys[2] - f_u).max() > 100 * ref.tolerance_p(f_u, c[None, :, 1] * x64, hp, den_p).max()


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    x = torch.zeros((4, 3000), dtype=torch.float32, device=DEV)
    c = torch.zeros((3000, 2), dtype=torch.float64, device=DEV)
    y = [torch.full((4, 1500), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    y1 = [torch.full((4, 3000), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]  # what q = 1 would write, were it let through
    h = torch.ones(1027, dtype=torch.float64, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    good = (ptr(x), 3000, 4, 3000, 2, ptr(c), ptr(h), ptr(h), 41, ptr(y[0]), ptr(y[1]), ptr(y[2]), 1500)

    def put(*pairs):
        args = list(good)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    cases = {
        "q 1": put((4, 1), (9, ptr(y1[0])), (10, ptr(y1[1])), (11, ptr(y1[2])), (12, 3000)),
        "q 33": put((4, 33)),
        "n_taps 40": put((8, 40)),
        "n_taps 0": put((8, 0)),
        "n_taps 1027": put((8, 1027)),
        "D 0": put((2, 0)),
        "T 0": put((3, 0)),
        "ld_x < T": put((1, 2999)),
        "ld_y < T_out": put((12, 1499)),
        "y_t is x": put((0, ptr(y[0])), (1, 1500), (3, 1500), (12, 750)),
        "y_q is x": put((0, ptr(y[1])), (1, 1500), (3, 1500), (12, 750)),
        "y_u is x": put((0, ptr(y[2])), (1, 1500), (3, 1500), (12, 750)),
        "y_q is y_u": put((10, ptr(y[2]))),
        "null x": put((0, None)),
        "null carrier": put((5, None)),
        "null taps_p": put((7, None)),
        "null taps_t with y_t": put((6, None)),
        "null y_q": put((10, None)),
        "null y_u": put((11, None)),
    }
    for name, args in cases.items():
        assert lib.mrx_tod_demodulate(hd, *args) == -1, name
        assert b"mrx_tod_demodulate" in lib.mrx_last_error(hd), name
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in y + y1)
    assert lib.mrx_tod_demodulate(hd, *good) == 0
    assert lib.mrx_tod_demodulate(hd, *put((6, None), (9, None))) == 0  # polarisation only needs no hT
    m = (ptr(x), ptr(x), ptr(x), 3000, 4, 3000, ptr(c), ptr(y1[0]), 3000)
    mod = {"null i": (None,) + m[1:], "null carrier": m[:6] + (None,) + m[7:], "null out": m[:7] + (None, 3000), "D 0": m[:4] + (0,) + m[5:],
           "T 0": m[:5] + (0,) + m[6:], "ld_in < T": m[:3] + (2999,) + m[4:], "ld_out < T": m[:8] + (2999,),
           "out is c": (ptr(y1[1]), ptr(y1[0]), ptr(x)) + m[3:], "in place at another pitch": (ptr(y1[0]), ptr(x), ptr(x), 3000, 4, 2000, ptr(c), ptr(y1[0]), 2500)}
    for name, args in mod.items():
        assert lib.mrx_tod_hwp_modulate(hd, *args) == -1, name
        assert b"mrx_tod_hwp_modulate" in lib.mrx_last_error(hd), name
    torch.cuda.synchronize()
    assert bool((y1[0] == 7.0).all())


def strided(a, pitch, offset, fill):
    """(buffer, [D, T] view at row pitch ``pitch``, ``offset`` words in) holding the float32 array ``a``."""
    import torch

    D, T = a.shape
    buf = torch.full((offset + D * pitch + 64,), fill, dtype=torch.float32, device=DEV)
    view = torch.as_strided(buf, (D, T), (pitch, 1), offset)
    view.copy_(torch.as_tensor(a))
    return buf, view


@pytest.mark.parametrize("D,T", [(1, 1), (3, 5), (7, 1023), (5, 1024), (4, 4099), (66, 2050)])
def test_modulate_against_numpy(gpu_ctx, D, T):
    """Out of place and in place, at 16-byte-aligned pitches and at odd ones a word in, T no multiple of 4: within
    2^-24 (|i| + |c| + |s|) of the float64 expression (one rounding to float32, and the float64 roundings far below it);
    nothing outside the rows is written; with c = s = 0 the result is i bit for bit."""
    import torch

    from maria_amd import hwp

    rng = np.random.default_rng(D + T)
    si, sc, ss = ((rng.standard_normal((D, T)) * k).astype(np.float32) for k in (3.0, 1e-2, 1e-2))
    c = hwp.carrier(rng.uniform(0, 2 * np.pi, T))
    want = ref.modulate(si, sc, ss, c)
    tol = 2.0**-24 * (np.abs(si) + np.abs(sc) + np.abs(ss)) * (1 + 1e-6)
    dc = torch.as_tensor(c).to(DEV)
    for pitch, offset in ((T + (-T) % 4, 0), (T + 3, 1)):
        (bi, vi), (bc, vc), (bs, vs) = (strided(a, pitch, offset, -3.0) for a in (si, sc, ss))
        keep = [b.clone() for b in (bi, bc, bs)]
        bo, vo = strided(np.zeros_like(si), pitch + 4, offset, 7.0)
        vo.fill_(7.0)
        out = hwp.modulate(vi, vc, vs, dc, out=vo, ctx=gpu_ctx)
        torch.cuda.synchronize()
        assert out is vo and all(torch.equal(a, b) for a, b in zip((bi, bc, bs), keep)), "an input changed"
        got = vo.cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - want) <= tol), (pitch, offset)
        vo.fill_(7.0)
        assert bool((bo == 7.0).all()), "written outside the rows"
        again = hwp.modulate(vi, vc, vs, dc, out=vi, ctx=gpu_ctx)  # in place
        torch.cuda.synchronize()
        assert again is vi and np.array_equal(vi.cpu().numpy().view(np.uint32), got.view(np.uint32)), "in place differs"
        vi.fill_(-3.0)
        assert bool((bi == -3.0).all()), "written outside the rows"
        vi.copy_(torch.as_tensor(si))
        (_, z1), (_, z2) = (strided(np.zeros_like(si), pitch, offset, -3.0) for _ in range(2))
        same = hwp.modulate(vi, z1, z2, dc, ctx=gpu_ctx)  # out=None
        assert tuple(same.shape) == (D, T) and np.array_equal(same.cpu().numpy().view(np.uint32), si.view(np.uint32)), "c = s = 0 changes i"


def small_sim(gamma, sky, hwp=None, T=2001):
    """19 positions behind a beam-free dish, 2001 samples at 200 Hz, pW, no atmosphere, no noise: the TOD."""
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation

    band = Band(center=150e9, width=30e9, name="f150")
    dets = Detectors(synthetic.hex_pack(19, np.radians(0.4)), [band], np.zeros(19, int), primary_size=1000.0, gamma=gamma)
    t = 1.7e9 + np.arange(T) / 200.0
    az, el = synthetic.daisy_scan(t, radius_deg=0.25, az_deg=120.0, el_deg=55.0)
    sim = Simulation(Instrument(dets), Plan(t, az, el), Site(altitude=5190.0), map=sky, noise=False, device_output=True, hwp=hwp)
    (tod,) = sim.run(units="pW")
    return tod


def blob_sky(planes, stokes):
    from maria_amd import map as mmap

    n = 64
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    blobs = {"I": 3e-3 * np.exp(-((X - 0.1) ** 2 + (Y + 0.2) ** 2) / 0.18), "Q": 2e-3 * np.exp(-((X + 0.2) ** 2 + (Y - 0.1) ** 2) / 0.18),
             "U": -1e-3 * np.exp(-((X - 0.15) ** 2 + (Y - 0.15) ** 2) / 0.18)}
    data = np.stack([blobs[s] if s in planes else np.zeros((n, n)) for s in stokes])[:, None].astype(np.float32)
    return mmap.ProjectionMap(data, nu=150e9, stokes=stokes, width=1.0, center=(120.0, 55.0), frame="az/el")


def test_simulation_behind_a_half_wave_plate(gpu_ctx):
    """The map field is S_I + S_c cos 4 chi + S_s sin 4 chi: with an I-only map the bits of the run without a plate; with a
    Q / U-only map float32(S_c cos + S_s sin) within 2^-23 (|S_c| + |S_s|), S_c and S_s from two runs without a plate whose
    detectors have gamma replaced by -gamma and pi / 4 - gamma; an unpolarised row sees nothing of Q and U."""
    from maria_amd import hwp

    gamma = np.radians([0.0, 45.0, 90.0, 135.0, 20.0])[np.arange(19) % 5]
    gamma[7] = np.nan
    plate = hwp.HWP(frequency=2.0, phase=0.3)
    host = lambda tod: tod.data["map"].cpu().numpy()  # noqa: E731
    for sky in (blob_sky("I", "I"), blob_sky("I", "IQU")):
        plain, turned = small_sim(gamma, sky), small_sim(gamma, sky, hwp=plate)
        assert "hwp" not in plain.metadata and turned.metadata["hwp"] == {"frequency": 2.0, "phase": 0.3, "direction": 1}
        assert np.abs(host(plain)).max() > 0
        np.testing.assert_array_equal(host(turned), host(plain))
    sky = blob_sky("QU", "IQU")
    turned = small_sim(gamma, sky, hwp=plate)
    assert turned.units == "pW" and turned.fields == ["map"]
    s_c = host(small_sim(-gamma, sky)).astype(np.float64)
    s_s = host(small_sim(np.pi / 4 - gamma, sky)).astype(np.float64)
    assert np.abs(s_c).max() > 0 and np.abs(s_s).max() > 0
    c = hwp.carrier(plate.angle(turned.coords.t))
    want = s_c * c[None, :, 0] + s_s * c[None, :, 1]
    err = np.abs(host(turned).astype(np.float64) - want)
    tol = 2.0**-23 * (np.abs(s_c) + np.abs(s_s))
    print(f"max |map field - (S_c cos + S_s sin)| / (2^-23 (|S_c| + |S_s|)) = {(err[tol > 0] / tol[tol > 0]).max():.3f}")
    assert np.all(err <= tol)
    assert np.all(host(turned)[7] == 0) and np.abs(host(turned)[6]).max() > 0


def hand_tod(D=6, T=3001, fs=200.0, seed=0):
    """A two-field TOD built by hand (one numpy field, one device-tensor field) with flags, detectors 1 and 4 unpolarised."""
    import torch

    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t, radius_deg=0.3)
    gamma = np.array([0.0, np.nan, 0.7, np.pi / 2, np.nan, -0.4])[:D]
    dets = Detectors(synthetic.hex_pack(D, np.radians(0.4)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int), gamma=gamma)
    rng = np.random.default_rng(seed)
    data = {"map": (rng.standard_normal((D, T)) + 5).astype(np.float32),
            "noise": torch.as_tensor(rng.standard_normal((D, T)).astype(np.float32)).to(DEV)}
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    flags[2, 1000:1003] = 1
    flags[1, 40] = 1
    return TOD(data, dets, Coordinates(t, az, el, offsets=dets.offsets), units="K_RJ", metadata={"latitude": -23.0, "longitude": -67.8}, flags=flags)


def test_tod_demodulate(gpu_ctx):
    import torch

    from maria_amd import downsample, hwp
    from maria_amd.flagging import downsample_flags

    tod = hand_tod()
    D, T, fs, f = 6, 3001, 200.0, 4.0
    plate = hwp.HWP(frequency=f, phase=0.2)
    kept = {k: (v.clone() if isinstance(v, torch.Tensor) else v.copy()) for k, v in tod.data.items()}
    t0, az0, el0, flags0 = tod.coords.t.copy(), tod.coords._baz.copy(), tod.coords._bel.copy(), tod.flags.clone()
    tod._calibrator = lambda data, to_krj: data  # a TOD that could convert units
    with pytest.raises(ValueError):
        tod.demodulate(ctx=gpu_ctx)  # no plate given, none in the metadata
    low = tod.demodulate(plate, ctx=gpu_ctx)
    q = min(32, hwp.max_factor(fs, f))
    assert q == 20
    h = hwp.design_taps((T - 1) / (t0[-1] - t0[0]), f)  # the rate as the time stamps give it
    T_out = downsample.output_length(T, q)
    pol = np.array([0, 2, 3, 5])
    idx = np.concatenate([np.arange(D), pol, pol])
    c = hwp.carrier(plate.angle(t0))
    assert low is not tod and low.fields == tod.fields == ["map", "noise"]
    for name in low.fields:
        v = low.data[name]
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (D + 8, T_out)
        x = kept[name].cpu().numpy() if isinstance(kept[name], torch.Tensor) else kept[name]
        r_t, r_q, r_u, den_t, den_p = ref.demodulate(x, c, q, h, h)
        got = v.cpu().numpy()
        x64 = x.astype(np.float64)
        assert np.all(np.abs(got[:D] - r_t) <= ref.tolerance_t(r_t, x, h, den_t))
        assert np.all(np.abs(got[D:D + 4] - r_q[pol]) <= ref.tolerance_p(r_q, c[None, :, 0] * x64, h, den_p)[pol])
        assert np.all(np.abs(got[D + 4:] - r_u[pol]) <= ref.tolerance_p(r_u, c[None, :, 1] * x64, h, den_p)[pol])
    np.testing.assert_array_equal(low.coords.t, t0[::q])
    np.testing.assert_array_equal(low.coords._baz, az0[::q])
    np.testing.assert_array_equal(low.coords._bel, el0[::q])
    np.testing.assert_array_equal(low.coords.offsets, tod.coords.offsets[idx])
    want = hwp.demodulated_detectors(tod.dets)
    assert low.dets.n == D + 8
    np.testing.assert_array_equal(low.dets.stokes_rows(), want.stokes_rows())
    np.testing.assert_array_equal(low.dets.gamma, want.gamma)
    np.testing.assert_array_equal(low.dets.offsets, tod.dets.offsets[idx])
    assert low.units == tod.units == "K_RJ" and low.metadata["latitude"] == -23.0
    meta = low.metadata["demodulate"]
    assert meta["f_hwp"] == f and meta["factor"] == q and meta["n_taps"] == h.size and meta["sample_rate"] == pytest.approx(fs / q, rel=1e-6)
    assert meta["rows"] == {"T": (0, D), "Q": (D, D + 4), "U": (D + 4, D + 8)}
    assert torch.equal(low.flags, downsample_flags(flags0, q)[torch.as_tensor(idx).to(DEV)]) and int(low.flags.sum()) > 0
    # an explicit factor and taps, and the plate from the metadata
    tod.metadata["hwp"] = plate.to_metadata()
    other = tod.demodulate(q=8, taps_p=scipy.signal.firwin(41, 0.1), ctx=gpu_ctx)
    assert other.metadata["demodulate"]["factor"] == 8 and other.metadata["demodulate"]["n_taps"] == 41 and other.coords.t.size == 376
    del tod.metadata["hwp"]
    # the source is as it was
    assert "demodulate" not in tod.metadata and tod.fields == ["map", "noise"] and torch.equal(tod.flags, flags0)
    for name, v in kept.items():
        same = torch.equal(tod.data[name], v) if isinstance(v, torch.Tensor) else np.array_equal(tod.data[name], v)
        assert same, name
    np.testing.assert_array_equal(tod.coords.t, t0)
    assert tod.to("pW") is not None  # the source converts ...
    with pytest.raises(NotImplementedError):  # ... the demodulated TOD carries no calibrator
        low.to("pW")
    with pytest.raises(ValueError):  # and is not demodulated again
        low.demodulate(plate, ctx=gpu_ctx)


def test_a_mapper_takes_the_stokes_rows_of_a_demodulated_tod(gpu_ctx):
    """MaximumLikelihoodMapper(stokes="IQU") on a demodulated TOD built by hand (T rows, Q rows, U rows under the
    Stokes-row override) against the same mapper on the equivalent plain TOD: detectors at -gamma and pi / 4 - gamma with
    the same Q / U-only signal.  Eight positions carry the four angles 0, 45, 90, 135 degrees each, so in every pixel the
    plain table's I column is orthogonal to its Q and U columns (sum cos 2 g = sum sin 2 g = 0 over a position's four
    rows at every sample) and both mappers solve the same Q / U equations: all three planes are finite in the same
    pixels, and the Q and U planes agree within 4 * 2^-23 max|tod| (float32 maps of equal float64 solutions)."""
    from maria_amd import hwp, synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.mappers import MaximumLikelihoodMapper
    from maria_amd.sim import TOD, Coordinates

    npos, T = 8, 4001
    D = 4 * npos
    t = 1.7e9 + np.arange(T) / 50.0
    az, el = synthetic.daisy_scan(t, radius_deg=0.3)
    gamma = np.tile(np.radians([0.0, 45.0, 90.0, 135.0]), npos)
    offsets = np.repeat(synthetic.hex_pack(npos, np.radians(0.4)), 4, axis=0)
    band = [Band(center=150e9, width=30e9, name="f150")]
    dets = Detectors(offsets, band, np.zeros(D, int), gamma=gamma)
    demod = hwp.demodulated_detectors(dets)
    # a smooth Q / U signal, one function of time per position, seen through the rows' own weights; nothing in the T rows
    Q = 1e-3 * np.sin(3 * az[None] + 40 * offsets[:, :1])
    U = -2e-3 * np.cos(2 * el[None] + 30 * offsets[:, 1:])
    rows = demod.stokes_rows()[D:] / 0.5  # K_RJ: over the detectors' I weight
    signal = (rows[:, 1:2] * np.concatenate([Q, Q]) + rows[:, 2:3] * np.concatenate([U, U])).astype(np.float32)
    meta = {"latitude": -23.0, "longitude": -67.8}
    full = TOD({"map": np.concatenate([np.zeros((D, T), np.float32), signal])}, demod,
               Coordinates(t, az, el, offsets=demod.offsets), units="K_RJ", metadata=dict(meta))
    plain_dets = Detectors(demod.offsets[D:], band, np.zeros(2 * D, int), gamma=demod.gamma[D:])
    plain = TOD({"map": signal}, plain_dets, Coordinates(t, az, el, offsets=plain_dets.offsets), units="K_RJ", metadata=dict(meta))
    kw = dict(center=(float(np.degrees(az.mean())), float(np.degrees(el.mean()))), width=0.9, resolution=0.05, stokes="IQU", nu=150e9,
              frame="az/el", units="K_RJ", noise_weights="uniform")
    a = MaximumLikelihoodMapper([full], **kw).run().data
    b = MaximumLikelihoodMapper([plain], **kw).run().data
    np.testing.assert_array_equal(np.isfinite(a), np.isfinite(b))
    bound = 4 * 2.0**-23 * np.abs(signal).max()
    for s in (1, 2):
        ok = np.isfinite(b[s])
        assert ok.sum() > 100 and np.abs(b[s][ok]).max() > 1e-4
        err = np.abs(a[s][ok].astype(np.float64) - b[s][ok]).max()
        print(f"plane {'IQU'[s]}: max |map - map of the plain TOD| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_end_to_end_recovers_an_iqu_sky(gpu_ctx):
    """61 positions x 1 polarised band behind a beam-free dish, gamma in {0, 45, 90, 135} degrees, a 60 s daisy at 400 Hz,
    HWP(8 Hz), no atmosphere, no noise; a 64^2 IQU sky of three smooth Gaussian blobs (sigma 0.3 of the half-width, different
    centres, peaks of a few mK: at the daisy's 0.5 deg / s far inside the 4 Hz pass band).  tod.demodulate(), then
    MaximumLikelihoodMapper(stokes="IQU") on the input grid: per Stokes plane the hit-weighted rms residual is below 1 % of
    that plane's peak (the bound test_recover_map_at_the_reduced_rate puts beside the reference's own), printed beside that
    of the same sky mapped from a run without a plate (DESIGN 3.27 holds both).  Then an unpolarised drift
    5 + 0.5 sin(2 pi 0.05 t), atmosphere-like, added to every row before demodulating: the Q and U series move by at most
    2 * 10^(-120 / 20) * max|x|, the design's stop-band claim times the mixing's 2, at every output whose window lies within
    the row (the (n_taps - 1) / 2 q outputs at either end have truncated, renormalised taps, which have no stop band: there
    the drift moved Q and U by up to 1.9 when this was measured)."""
    import torch

    from maria_amd import hwp, synthetic
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.mappers import MaximumLikelihoodMapper
    from maria_amd.sim import TOD, Plan, Simulation, sky_transform_stack
    from oracle import mapsample

    npos, width, n = 61, 1.0, 64
    res = width / (n - 1)
    gamma = np.radians([0.0, 45.0, 90.0, 135.0])[np.arange(npos) % 4]
    dets = Detectors(synthetic.hex_pack(npos, np.radians(width / 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(npos, int),
                     primary_size=1000.0, gamma=gamma)
    plan = Plan.daisy(start_time=1.7e9, duration=60.0, sample_rate=400.0, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
    site = Site(altitude=5190.0)
    phi, theta = mapsample.frame_angles(plan.phi.astype(np.float32)[None], plan.theta.astype(np.float32)[None],
                                        sky_transform_stack(plan.time, site.latitude, site.longitude))
    xyz = mapsample.phi_theta_to_xyz(phi[0], theta[0]).astype(float).mean(axis=0)
    xyz /= np.linalg.norm(xyz)
    centre = (float(np.arctan2(xyz[1], xyz[0]) % (2 * np.pi)), float(np.arcsin(xyz[2])))
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    blob = lambda peak, x0, y0: peak * np.exp(-((X - x0) ** 2 + (Y - y0) ** 2) / (2 * 0.3**2))  # noqa: E731
    data = np.stack([blob(4e-3, 0.1, -0.05), blob(2e-3, -0.15, 0.1), blob(-3e-3, 0.05, 0.2)])[:, None].astype(np.float32)
    sky = mmap.ProjectionMap(data, nu=150e9, stokes="IQU", width=width, center=np.degrees(centre), frame="ra/dec")
    kw = dict(center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="IQU", nu=150e9, frame="ra/dec", units="K_RJ",
              noise_weights="uniform")
    residual = {}
    for name, plate in (("hwp", hwp.HWP(frequency=8.0)), ("plain", None)):
        (tod,) = Simulation(Instrument(dets), plan, site, map=sky, noise=False, device_output=True, hwp=plate).run()
        assert tod.units == "K_RJ" and tod.fields == ["map"]
        if plate is not None:
            full = tod
            tod = demod = tod.demodulate(ctx=gpu_ctx)
            # (at 1.7e9 s the plan's step rounds to 2^-22 s: its rate is 399.991 Hz, and the largest factor 19, not 20)
            q = tod.metadata["demodulate"]["factor"]
            assert q == hwp.max_factor((plan.time.size - 1) / (plan.time[-1] - plan.time[0]), 8.0) and q in (19, 20)
            assert tod.coords.t.size == -(-plan.time.size // q) and tod.dets.n == 3 * npos
        mapper = MaximumLikelihoodMapper([tod], **kw)
        out = mapper.run()
        assert out.data.shape == sky.data.shape and np.allclose(out.xi, sky.xi, atol=1e-12) and np.allclose(out.eta, sky.eta, atol=1e-12)
        solved = np.isfinite(out.data[:, 0])
        assert solved.all(axis=0).mean() > 0.3
        w = mapper.products["weight"][0, 0]  # H[0, 0]: the hits, as the reference weighs its residual
        residual[name] = np.array([np.sqrt(np.sum(w[solved[s]] * (out.data[s, 0][solved[s]] - sky.data[s, 0][solved[s]]) ** 2) / np.sum(w[solved[s]]))
                                   for s in range(3)])
    peaks = np.abs(sky.data[:, 0]).max(axis=(-1, -2))
    print("weighted rms residual per Stokes plane [K_RJ]: demodulated", residual["hwp"], "without a plate", residual["plain"], "peaks", peaks)
    assert np.all(residual["hwp"] < 0.01 * peaks)
    # the unpolarised drift under Q and U
    t = full.coords.t - full.coords.t[0]
    drift = torch.as_tensor((5 + 0.5 * np.sin(2 * np.pi * 0.05 * t)).astype(np.float32)).to(DEV)
    loaded = TOD({"map": full.data["map"] + drift[None]}, full.dets, full.coords, units=full.units, metadata=dict(full.metadata))
    # (in the interior: an output whose window is cut by the row's end has taps renormalised, and those have no stop band)
    H = (demod.metadata["demodulate"]["n_taps"] - 1) // 2
    j = np.arange(demod.coords.t.size)
    inner = torch.as_tensor((j * q >= H) & (j * q < t.size - H)).to(DEV)
    assert int(inner.sum()) > 1000
    moved = (loaded.demodulate(ctx=gpu_ctx).data["map"] - demod.data["map"])[npos:][:, inner].abs().max().item()
    bound = 2 * 10 ** (-120 / 20) * float(loaded.data["map"].abs().max())
    print(f"an unpolarised 5 + 0.5 sin drift moves Q and U by at most {moved:.3e}, bound {bound:.3e}")
    assert moved <= bound


def test_remove_hwpss_against_lstsq(gpu_ctx):
    """Harmonics 1 and 2 injected into a TOD without sky polarisation, then TOD.remove_hwpss: metadata["regress"]
    ["coefficients"] against numpy.linalg.lstsq on the same float32 templates, within the bound tests/test_gpu_regress.py
    holds TOD.regress to (1e3 K T eps max|a|), and the injected amplitudes come back."""
    from maria_amd import hwp

    tod = hand_tod(seed=3)
    tod.flags = None
    D, T = 6, 3001
    plate = hwp.HWP(frequency=2.0, phase=0.1)
    tod.metadata["hwp"] = plate.to_metadata()
    amps = {1: (0.3, np.linspace(-0.2, 0.2, D)), 2: (np.linspace(0.05, 0.1, D), -0.04)}
    dirty = hwp.inject_hwpss(tod, amps, ctx=gpu_ctx)
    assert np.array_equal(tod.data["map"], hand_tod(seed=3).data["map"])  # the source is as it was
    B = hwp.harmonic_templates(plate.angle(tod.coords.t), (1, 2))
    fields = [v.cpu().numpy() for v in dirty.data.values()]
    signal = (fields[0] + fields[1]).astype(np.float64)  # the float32 sum of the fields, as TOD.regress forms it
    a = np.linalg.lstsq(B.astype(np.float64).T, signal.T, rcond=None)[0].T
    clean = dirty.remove_hwpss((1, 2), ctx=gpu_ctx)
    coef = clean.metadata["regress"]["coefficients"]
    assert coef.shape == (D, 4) and clean.metadata["hwpss"] == {"harmonics": (1, 2)} and clean.metadata["regress"]["failed_rows"].size == 0
    err = np.abs(coef - a).max()
    bound = 1e3 * 4 * T * 2.0**-52 * np.abs(a).max()
    print(f"max |coefficients - lstsq| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    injected = np.stack([np.broadcast_to(np.asarray(amps[k][j], float), (D,)) for k in (1, 2) for j in (0, 1)], axis=1)
    assert np.abs(coef - injected).max() < 0.1  # (noise of sigma 1.4 over 3001 samples: 0.04 a coefficient)
    with pytest.raises(ValueError):
        dirty.remove_hwpss((1, 2, 3, 4, 5), ctx=gpu_ctx)
