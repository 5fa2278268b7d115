"""mrx_tod_onepole, mrx_tod_onepole_inverse, maria_amd.time_constants, the simulation's lag and
TOD.deconvolve_time_constants on the device, against the numpy float64 reference of tests/timeconst_ref.py.

The lag is held to |y - y64| <= 2^-24 |y64| + 64 2^-53 max|x| / (1 - a) on every sample: the float32 store, and the float64
roundings of a time-parallel evaluation (every intermediate is a convex combination of samples, each rounding enters
once and is damped by powers of a, a sum <= 1 / (1 - a); a power a^k with relative error k 2^-53 multiplies a carry, and
k a^k <= 1 / (e (1 - a)); 64 is headroom over the handful of roundings a composition has).  The inverse is compared bit
for bit, and inverse(lag(x)) to 2^-24 |x| + (1 + a) / (1 - a) 2^-23 max|y|: the float32 rounding of the two stored samples
the FIR reads, amplified by its gain, with a factor 2 of headroom."""

import numpy as np
import pytest
import timeconst_ref as ref
from test_gpu_downsample import _centre
from test_gpu_flagging import device_rows, untouched_outside
from test_gpu_subscans import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INIT = {0: "zero", 1: "steady"}
LONG = 33797  # 34 tiles: three work items of the inverse out of place, a single one in place


def run(gpu_ctx, entry, x, a, init, layout):
    """``entry`` ("apply" or "deconvolve") of the host array ``x`` in one of the layouts: "plain" (new output), "padded"
    (padded pitches in buffers that start one and three elements off alignment; nothing may be written outside), "in place"
    and "in place, padded".  Returns the result on the host; the input must not change where the call is out of place."""
    import torch

    from maria_amd import time_constants

    fn = getattr(time_constants, entry)
    x = np.array(x)  # (the cases' arrays are read-only)
    T = x.shape[1]
    d_a = torch.as_tensor(np.array(a)).to(DEV)
    if layout == "plain":
        dx = torch.as_tensor(np.asarray(x)).to(DEV)
        out = fn(dx, d_a, init=INIT[init], ctx=gpu_ctx)
        assert out is not dx and np.array_equal(bits(dx.cpu().numpy()), bits(x))
        return out.cpu().numpy()
    if layout == "in place":
        dx = torch.as_tensor(np.asarray(x)).to(DEV)
        assert fn(dx, d_a, init=INIT[init], out=dx, ctx=gpu_ctx) is dx
        return dx.cpu().numpy()
    xbuf, xv = device_rows(x, T + 3, 1, -3.0)
    if layout == "in place, padded":
        assert fn(xv, d_a, init=INIT[init], out=xv, ctx=gpu_ctx) is xv
        got = xv.cpu().numpy()
        assert untouched_outside(xbuf, xv, -3.0), "written past T"
        return got
    assert layout == "padded"
    before = xbuf.clone()
    ybuf, yv = device_rows(np.zeros_like(x), T + 5, 3, 7.0)
    yv.fill_(7.0)
    assert fn(xv, d_a, init=INIT[init], out=yv, ctx=gpu_ctx) is yv
    torch.cuda.synchronize()
    assert torch.equal(xbuf, before), "the input changed"
    got = yv.cpu().numpy()
    assert untouched_outside(ybuf, yv, 7.0), "written past T"
    return got


LAYOUTS = ["plain", "padded", "in place", "in place, padded"]


@pytest.mark.parametrize("D", ref.ROWS)
def test_the_lag_against_the_reference(gpu_ctx, D):
    """Every T, both init, every sample: inside the bound; rows with a = 0 are the input's bits.  The layouts take turns."""
    worst = 0.0
    for i, T in enumerate(ref.TIMES):
        x, a = ref.case(D, T)
        for init in (0, 1):
            y64 = ref.case_forward64(D, T, init)
            got = run(gpu_ctx, "apply", x, a, init, LAYOUTS[(i + init + D) % 4])
            assert got.dtype == np.float32 and got.shape == (D, T)
            err, bound = np.abs(got.astype(np.float64) - y64), ref.forward_bound(y64, x, a)
            print(f"D {D} T {T} init {init}: max |y - y64| / bound = {(err / bound).max():.3f}")
            assert np.all(err <= bound), (D, T, init, int((err > bound).sum()))
            assert np.array_equal(bits(got[a == 0.0]), bits(x[a == 0.0]))
            worst = max(worst, float((err / bound).max()))
    print(f"D {D}: max |y - y64| / bound = {worst:.3f}")


@pytest.mark.parametrize("D", ref.ROWS)
def test_the_inverse_bit_for_bit(gpu_ctx, D):
    """The same grid and one longer row set (more than one work item a row out of place), every layout in turn: the bits
    of the float64 lines of the header."""
    for i, T in enumerate(ref.TIMES + [LONG]):
        y, a = ref.case(D, T)
        for init in (0, 1):
            want = ref.inverse(y, a, init)
            for layout in (LAYOUTS if T in (5, 1025, LONG) else [LAYOUTS[(i + init + D) % 4], LAYOUTS[(i + init + D + 2) % 4]]):
                got = run(gpu_ctx, "deconvolve", y, a, init, layout)
                assert np.array_equal(bits(got), bits(want)), (D, T, init, layout, int((bits(got) != bits(want)).sum()))


@pytest.mark.parametrize("D", ref.ROWS)
def test_the_round_trip(gpu_ctx, D):
    worst = 0.0
    for i, T in enumerate(ref.TIMES):
        x, a = ref.case(D, T)
        for init in (0, 1):
            y = run(gpu_ctx, "apply", x, a, init, LAYOUTS[(i + init) % 4])
            back = run(gpu_ctx, "deconvolve", y, a, init, LAYOUTS[(i + init + 1) % 4])
            err, bound = np.abs(back.astype(np.float64) - x), ref.round_trip_bound(x, y, a)
            assert np.all(err <= bound), (D, T, init, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    print(f"D {D}: max |inverse(lag(x)) - x| / bound = {worst:.3f}")


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0, 5.0], np.float32)


@pytest.mark.parametrize("entry", ["mrx_tod_onepole", "mrx_tod_onepole_inverse"])
def test_rows_without_a_pole_are_copied(gpu_ctx, entry):
    """a = 0, and through the C entry (the Python layer refuses them) a outside [0, 1), infinite or NaN: the row is the
    input's bits, signed zeros, denormals and the largest float32 included, out of place and in place, both init; the row
    with a pole between them is not."""
    import torch

    from maria_amd._lib import ptr

    poles = np.array([0.0, 1.0, -0.5, np.nan, 0.5, np.inf, -np.inf, 1.5, -0.0, 1.0 + 2.0**-52])
    D = len(poles)
    rng = np.random.default_rng(3)
    for T in (1, 7, 1024, 2051):
        x = rng.permutation(np.tile(SPECIAL, (D, -(-T // len(SPECIAL))))[:, :T], axis=1).astype(np.float32)
        d_a = torch.as_tensor(poles).to(DEV)
        for init in (0, 1):
            xbuf, xv = device_rows(x, T + 3, 1, -3.0)
            ybuf, yv = device_rows(np.zeros_like(x), T + 5, 3, 7.0)
            gpu_ctx.call(entry, ptr(xv), T + 3, D, T, ptr(d_a), init, ptr(yv), T + 5)
            got = yv.cpu().numpy()
            copied = np.arange(D) != 4
            assert np.array_equal(bits(got[copied]), bits(x[copied])), (T, init)
            assert T < 7 or not np.array_equal(bits(got[4]), bits(x[4]))
            assert untouched_outside(ybuf, yv, 7.0)
            gpu_ctx.call(entry, ptr(xv), T + 3, D, T, ptr(d_a), init, ptr(xv), T + 3)
            assert np.array_equal(bits(xv.cpu().numpy()), bits(got)), (T, init)
            assert untouched_outside(xbuf, xv, -3.0)


def test_constant_rows_stay_constant(gpu_ctx):
    """init "steady" on a constant row: y64 is the constant, at any length, so the result is within the bound of it."""
    for T in (1, 1023, 4099, 50021):
        a = np.array(ref.POLES + [1.0 - 2.0**-20])
        c = np.array([5.0, -3.25, 1e6, 0.1, 1e-3, 77.7, 12345.678], np.float32)
        x = np.repeat(c[:, None], T, axis=1)
        got = run(gpu_ctx, "apply", x, a, 1, "plain")
        y64 = x.astype(np.float64)
        err = np.abs(got.astype(np.float64) - y64)
        assert np.all(err <= ref.forward_bound(y64, x, a)), T
        assert np.array_equal(bits(got[0]), bits(x[0]))


@pytest.mark.parametrize("entry", ["apply", "deconvolve"])
def test_the_same_bits_whatever_else_is_in_the_call(gpu_ctx, entry):
    """A second call, every row computed alone, padded pitches off alignment, in place, and unrelated rows around: the
    bits of the plain call."""
    D = 33
    for T in (5, 1025, 4099, LONG):
        x, a = ref.case(D, T)
        for init in (0, 1):
            base = run(gpu_ctx, entry, x, a, init, "plain")
            for layout in LAYOUTS:
                assert np.array_equal(bits(run(gpu_ctx, entry, x, a, init, layout)), bits(base)), (T, init, layout)
            for d in range(D) if T == 1025 else (0, D // 2, D - 1):
                alone = run(gpu_ctx, entry, x[d : d + 1], a[d : d + 1], init, "padded" if d % 2 else "plain")
                assert np.array_equal(bits(alone[0]), bits(base[d])), (T, init, d)
            other, b = ref.case(3, T)
            more = run(gpu_ctx, entry, np.concatenate([other, x, other[::-1]]), np.concatenate([b, a, b[::-1]]), init, "padded")
            assert np.array_equal(bits(more[3 : 3 + D]), bits(base)), (T, init)


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the output untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T = 4, 3000
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    a = torch.full((D,), 0.5, dtype=torch.float64, device=DEV)
    y = torch.full((D, T + 4), 7.0, dtype=torch.float32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    good = (ptr(x), T, D, T, ptr(a), 1, ptr(y), T + 4)

    def put(*pairs):
        args = list(good)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    bad = {"null in": put((0, None)), "null a": put((4, None)), "null out": put((6, None)), "D 0": put((2, 0)), "D -1": put((2, -1)),
           "T 0": put((3, 0)), "T -1": put((3, -1)), "ld_in < T": put((1, T - 1)), "ld_out < T": put((7, T - 1)), "init 2": put((5, 2)),
           "init -1": put((5, -1)), "in place at another pitch": put((6, ptr(x)), (7, T + 4))}
    for entry in ("mrx_tod_onepole", "mrx_tod_onepole_inverse"):
        for name, args in bad.items():
            assert getattr(lib, entry)(hd, *args) == -1, (entry, name)
            assert entry.encode() in lib.mrx_last_error(hd), (entry, name)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) and bool((x == 1.0).all()), entry
    assert lib.mrx_tod_onepole(hd, *good) == 0 and lib.mrx_tod_onepole(hd, *put((5, 0))) == 0
    torch.cuda.synchronize()
    assert bool((y[:, T:] == 7.0).all()) and float(y[0, 0]) == 0.5 and float(y[0, 1]) == 0.75


# ---- the simulation ------------------------------------------------------------------------------------------------

SCAN = dict(start_time=1.7e9, duration=60.0, sample_rate=50.0, scan_center=(120.0, 55.0), throw=0.3, speed=0.5, accel=1.0)
TAUS = (30e-3, 12e-3)  # seconds, the two bands': 0.0086 and 0.0034 degrees on the sky at 0.29 degrees a second, the beams 0.0079 and 0.0049
N_PIX, WIDTH = 128, 1.0  # the map: pixels a side, degrees


def instrument(taus, keyword=True):
    from maria_amd.instrument import Band, Detectors, Instrument

    kw = [dict(time_constant=t) if keyword else {} for t in taus]
    bands = [Band(center=93e9, width=27e9, shape="top_hat", name="f093", **kw[0]), Band(center=150e9, width=41e9, shape="top_hat", name="f150", **kw[1])]
    return Instrument(Detectors.hexagon(32, WIDTH / 2, bands, primary_size=30.0))


def sky_and_plan():
    """Three compact sources (Gaussians of sigma 0.015 degrees, two pixels) under the back-and-forth scan."""
    from maria_amd import map as mmap
    from maria_amd.instrument import Site
    from maria_amd.sim import Plan, sky_transform_stack

    X, Y = np.meshgrid(np.linspace(-1, 1, N_PIX), np.linspace(-1, 1, N_PIX))
    data = sum(amp * np.exp(-((X - x0) ** 2 + (Y - y0) ** 2) / (2 * 0.03**2)) for amp, x0, y0 in ((5e-3, 0.0, 0.0), (-3e-3, 0.2, -0.1), (4e-3, -0.24, 0.16)))
    site = Site(altitude=5000.0)
    plan = Plan.back_and_forth(**SCAN)
    centre = _centre(plan.phi.astype(np.float32), plan.theta.astype(np.float32), sky_transform_stack(plan.time, site.latitude, site.longitude))
    sky = mmap.ProjectionMap(data.astype(np.float32), nu=150e9, width=WIDTH, center=np.degrees(centre), frame="ra/dec")
    return sky, plan, site, centre


def poles_of_the_run(tod):
    from maria_amd import time_constants

    return time_constants.poles(tod.dets.time_constant, time_constants.sample_rate_of(tod.coords.t))


def lag_by_hand(gpu_ctx, tod_pw, field, taus):
    """The tau = 0 run in pW with ``field`` through ``time_constants.apply`` and every other field as it is, then
    ``TOD.to("K_RJ")``: (the K_RJ fields, the lagged field in pW)."""
    import torch

    from maria_amd import time_constants
    from maria_amd.sim import TOD

    tau = np.repeat(taus, 32)
    a = time_constants.poles(tau, time_constants.sample_rate_of(tod_pw.coords.t))
    x = torch.as_tensor(tod_pw.data[field]).to(DEV, torch.float32)
    y = time_constants.apply(x, a, init="steady", ctx=gpu_ctx).cpu().numpy()
    by_hand = TOD(dict(tod_pw.data, **{field: y}), tod_pw.dets, tod_pw.coords, units="pW", metadata=dict(tod_pw.metadata))
    by_hand._calibrator = tod_pw._calibrator
    return by_hand.to("K_RJ").data, y


@pytest.fixture(scope="module")
def map_runs(gpu_ctx):
    """The map field of 32 positions x 2 bands on the back-and-forth scan, 3000 samples, no noise: lagged in K_RJ and in pW,
    tau = 0 in K_RJ and in pW, and built without the keyword in K_RJ."""
    from maria_amd.sim import Simulation

    sky, plan, site, centre = sky_and_plan()
    sim = lambda inst, **kw: Simulation(inst, plan, site, map=sky, noise=False, **kw)  # noqa: E731
    runs = {"lagged": sim(instrument(TAUS)).run()[0], "lagged pW": sim(instrument(TAUS)).run("pW")[0], "zero": sim(instrument((0.0, 0.0))).run()[0],
            "zero pW": sim(instrument((0.0, 0.0))).run("pW")[0], "no keyword": sim(instrument(TAUS, keyword=False)).run()[0],
            "halves": [sim(instrument(TAUS), shard=(r, 2)).run()[0] for r in (0, 1)], "centre": centre}
    return runs


def test_the_simulated_map_field_is_the_lag_of_the_unlagged_run(gpu_ctx, map_runs):
    """Bit for bit: the lagged run's "map" is the tau = 0 run in pW, lagged by hand, converted by TOD.to; the tau = 0 run is the
    run of an instrument built without the keyword, metadata included; a run of half the rows is those rows of the whole."""
    lagged, zero, plain = map_runs["lagged"], map_runs["zero"], map_runs["no keyword"]
    assert lagged.units == zero.units == "K_RJ" and lagged.fields == ["map"] and lagged.data["map"].shape == (64, 3000)
    assert lagged.metadata["time_constants"] == {"applied": True, "fields": ["map"], "init": "steady"}
    assert map_runs["lagged pW"].units == "pW" and map_runs["lagged pW"].metadata["time_constants"]["applied"]
    assert lagged.dets.time_constant.tolist() == [TAUS[0]] * 32 + [TAUS[1]] * 32
    want, _ = lag_by_hand(gpu_ctx, map_runs["zero pW"], "map", TAUS)
    assert np.array_equal(bits(lagged.data["map"]), bits(want["map"]))
    assert float(np.abs(lagged.data["map"] - zero.data["map"]).max()) > 0.05 * float(np.abs(zero.data["map"]).max())  # the lag is there
    assert "time_constants" not in zero.metadata and zero.metadata == plain.metadata
    assert np.array_equal(bits(zero.data["map"]), bits(plain.data["map"]))
    for r, half in enumerate(map_runs["halves"]):
        assert half.metadata["shard"]["rows"] == [32 * r, 32 * r + 32] and half.dets.time_constant.tolist() == [TAUS[r]] * 32
        assert half.metadata["time_constants"]["applied"]
        assert np.array_equal(bits(half.data["map"]), bits(lagged.data["map"][32 * r : 32 * r + 32]))


def test_the_simulated_atmosphere_field_is_the_lag_of_the_unlagged_run(gpu_ctx):
    """The same comparison for "atmosphere", with noise beside it: the noise is the law of the readout's output and is
    left as drawn, so the lagged run's is the tau = 0 run's, converted like the rest."""
    from maria_amd.instrument import Site
    from maria_amd.sim import Plan, Simulation

    plan, site = Plan.back_and_forth(**SCAN), Site(altitude=5000.0)
    kw = dict(atmosphere="2d", atmosphere_kwargs={"n_layers": 2, "seed": 4, "pwv_rms_frac": 0.1}, noise=True, noise_seed=11)
    (lagged,) = Simulation(instrument(TAUS), plan, site, **kw).run()
    (zero_pw,) = Simulation(instrument((0.0, 0.0)), plan, site, **kw).run("pW")
    assert lagged.units == "K_RJ" and lagged.fields == ["atmosphere", "noise"]
    assert lagged.metadata["time_constants"] == {"applied": True, "fields": ["atmosphere"], "init": "steady"}
    assert "time_constants" not in zero_pw.metadata and zero_pw.units == "pW"
    want, y_pw = lag_by_hand(gpu_ctx, zero_pw, "atmosphere", TAUS)
    assert not np.array_equal(y_pw, zero_pw.data["atmosphere"])
    for name in ("atmosphere", "noise"):
        assert np.array_equal(bits(lagged.data[name]), bits(want[name])), name


def test_tod_deconvolve_time_constants(gpu_ctx, map_runs):
    """On the simulated TOD (the run in pW, where the lag was applied): every field within the round-trip bound of the
    tau = 0 run's; flags grow by one sample; ``tau`` overrides the detectors'; ``into`` and the metadata; a downsampled TOD
    is refused."""
    import torch

    from maria_amd import time_constants
    from maria_amd.sim import TOD

    lagged, zero = map_runs["lagged pW"], map_runs["zero pW"]
    a = poles_of_the_run(lagged)
    y, x = lagged.data["map"], zero.data["map"]
    flags = np.zeros(y.shape, np.uint8)
    flags[0, 0] = flags[1, 2999] = flags[2, 10] = flags[2, 11] = 1
    flags[3, 100:103] = 2
    tod = TOD({"map": y, "other": torch.as_tensor(y).to(DEV)}, lagged.dets, lagged.coords, units="pW", metadata=dict(lagged.metadata),
              flags=torch.as_tensor(flags).to(DEV))
    tod._calibrator = lagged._calibrator
    out = tod.deconvolve_time_constants(ctx=gpu_ctx)
    assert out is not tod and out.fields == ["map", "other"] and out.units == "pW" and out.dets is tod.dets and out.coords is tod.coords
    assert out._calibrator is tod._calibrator and "deconvolved" not in tod.metadata["time_constants"] and np.array_equal(tod.data["map"], y)
    meta = out.metadata["time_constants"]
    assert meta["applied"] and meta["deconvolved"] is True and meta["deconvolved_init"] == "steady"
    assert meta["deconvolved_tau"].tolist() == lagged.dets.time_constant.tolist()
    bound = ref.round_trip_bound(x, y, a)
    for name in out.fields:
        v = out.data[name]
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32
        err = np.abs(v.cpu().numpy().astype(np.float64) - x)
        print(f"{name}: max |deconvolved - unlagged| / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound)
        assert np.array_equal(bits(v.cpu().numpy()), bits(ref.inverse(y, a, 1)))
    grown = flags.copy()
    grown[:, 1:] |= flags[:, :-1]
    assert np.array_equal(out.flags.cpu().numpy(), grown) and int(grown.astype(bool).sum()) == int(flags.astype(bool).sum()) + 3
    assert np.array_equal(tod.flags.cpu().numpy(), flags)
    plain = TOD({"map": y}, lagged.dets, lagged.coords, units="pW")
    assert plain.deconvolve_time_constants(ctx=gpu_ctx).flags is None
    # tau of one's own: a scalar, an array, and 0 (nothing is taken out)
    fs = time_constants.sample_rate_of(lagged.coords.t)
    for tau in (20e-3, np.linspace(1e-3, 40e-3, 64), 0.0):
        got = plain.deconvolve_time_constants(tau=tau, init="zero", into="map", ctx=gpu_ctx)
        want = ref.inverse(y, time_constants.poles(np.broadcast_to(tau, (64,)), fs), 0)
        assert np.array_equal(bits(got.data["map"].cpu().numpy()), bits(want))
        meta = got.metadata["time_constants"]
        assert sorted(meta) == ["deconvolved", "deconvolved_init", "deconvolved_tau"] and meta["deconvolved"] is True
        assert meta["deconvolved_init"] == "zero" and meta["deconvolved_tau"].tolist() == np.broadcast_to(tau, (64,)).tolist()
    assert np.array_equal(bits(got.data["map"].cpu().numpy()), bits(y))
    with pytest.raises(ValueError, match="into"):
        plain.deconvolve_time_constants(into="noise", ctx=gpu_ctx)
    low = TOD({"map": torch.as_tensor(y).to(DEV)}, lagged.dets, lagged.coords, units="pW").downsample(2, ctx=gpu_ctx)
    with pytest.raises(NotImplementedError, match="deconvolve first"):
        low.deconvolve_time_constants(ctx=gpu_ctx)


def test_the_map_through_the_lag(gpu_ctx, map_runs):
    """Compact sources under the back-and-forth scan with tau x scan speed above half a beam in both bands.  The lagged,
    the deconvolved and the tau = 0 TODs binned onto one grid: r_lag and r_dec, the rms differences from the tau = 0 map over the
    pixels hit in all three.  r_dec <= 0.01 r_lag: the round-trip bound puts r_dec at float32 rounding times a gain of order
    10, five orders below the signal, and r_lag is first order in tau x speed / beam, so the factor leaves three orders of
    margin on one side and fails where the deconvolution does nothing or has the wrong sign."""
    from maria_amd.mappers import BinMapper

    res = WIDTH / (N_PIX - 1)
    lagged, zero = map_runs["lagged"], map_runs["zero"]
    speed = SCAN["speed"] * np.cos(np.radians(SCAN["scan_center"][1]))  # degrees on the sky a second
    beams = np.degrees([lagged.dets.angular_fwhm()[0], lagged.dets.angular_fwhm()[-1]])
    assert all(t * speed >= 0.5 * b for t, b in zip(TAUS, beams)), (speed, beams)
    tods = {"lagged": lagged, "deconvolved": lagged.deconvolve_time_constants(ctx=gpu_ctx), "zero": zero}
    assert tods["deconvolved"].units == "K_RJ"
    maps = {}
    for name, tod in tods.items():
        mapper = BinMapper([tod], center=np.degrees(map_runs["centre"]), width=(N_PIX + 0.5) * res, resolution=res, stokes="I",
                           nu=[b.center for b in tod.dets.bands], frame="ra/dec", units="K_RJ")
        maps[name] = np.asarray(mapper.run().data[0, :], np.float64)
    hit = ~np.isnan(maps["lagged"]) & ~np.isnan(maps["deconvolved"]) & ~np.isnan(maps["zero"])
    assert hit.mean() > 0.05
    r_lag = float(np.sqrt(np.mean((maps["lagged"] - maps["zero"])[hit] ** 2)))
    r_dec = float(np.sqrt(np.mean((maps["deconvolved"] - maps["zero"])[hit] ** 2)))
    peak = float(np.abs(maps["zero"][hit]).max())
    print(f"r_lag = {r_lag:.3e} K_RJ, r_dec = {r_dec:.3e} K_RJ, r_dec / r_lag = {r_dec / r_lag:.2e}; the map's peak {peak:.3e} K_RJ")
    assert r_lag > 0 and r_lag > 100 * r_dec
    assert r_dec <= 0.01 * r_lag
