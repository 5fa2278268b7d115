"""mrx_tod_segment_moments, mrx_tod_segment_flag, maria_amd.cuts, TOD.stats and TOD.cut on the device, against
the numpy float64 reference of tests/cuts_ref.py.

Counts, min, max, empty and wholly flagged segments are exact everywhere.  Where every sum is exact in any order (small
integers on power-of-two lengths: tests/test_host_cuts.py proves it by summing forwards, backwards and with fsum) the
device is compared bit for bit.  On Gaussian data the bounds are derived, with u = 2^-53 and L the segment's length:

  sum, D2   A float64 sum of n <= L terms in any order is within (n - 1) u sum|terms| of the exact sum to first order, and
            the reference's fsum within half an ulp, u sum|terms| at most: (L + 1) u sum|terms| (the project's bound for a
            sum in any order).  D2's terms, a difference and a square, are the same float64 operations on both sides.
  mu        = sum / n, one division on either side: (L + 1) u sum|term| / n + u |mu|.  (The second division's half ulp is
            inside the first term: the device's sum is off by (n - 1) u sum|term| at most, not (L + 1), and
            sum|term| / n >= |mu|.)
  M_k       = sum e^k, e = term - mu with the side's own rounded mu.  Three first-order parts: the summation,
            (L + 1) u sum|e|^k; the roundings of a term (e once, entering k times, and the products),
            (k + 1) u sum|e|^k; and the mean: with mu off by dmu every e moves by dmu and e^k by k |e|^(k-1) dmu,
            k |dmu| sum|e|^(k-1) in all, |dmu| from mu's bound.  Second-order terms (dmu^2, u^2 L^2) are below L u < 2.3e-13
            of these for L <= 2049; a factor 1.001 stands for them.

tests/test_host_cuts.py shows what these bounds see: float32 accumulation, a float32 mean and one dropped sample."""

import cuts_ref as ref
import numpy as np
import pytest
from test_gpu_flagging import device_rows, untouched_outside
from test_gpu_subscans import LENGTHS, ROWS, TIMES, bits, make_bounds, rows, to_device
from test_host_cuts import (CUT_DETECTORS, DEAD, EXACT_CASES, NOISY, NOISY_SEGMENTS, defects, exact_rows, power_of_two_bounds,
                            reference_verdict)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("hits", "pairs") + ref.NAMES


def host(m):
    """The Moments of the device as a dict of numpy arrays."""
    return {k: getattr(m, k).cpu().numpy() for k in FIELDS}


def moments_case(gpu_ctx, D, T, seed, with_flags, with_model, padded):
    """One Gaussian case on the shapes of test_gpu_subscans.py against the reference: the exact quantities exactly, the
    sums within their bounds; returns the worst |got - ref| / bound."""
    import torch

    from maria_amd import cuts

    bounds = make_bounds(T, seed)
    x, model, flags = rows(D, T, 1000 * T + 10 * D + seed, exact=False)
    if T >= 64:
        flags[D - 1, bounds[1]:bounds[2]] = 2  # one segment wholly flagged in the last row
    bufs, (xv, mv, fv) = to_device(x, model, flags, padded)
    before = [b.clone() for b in bufs]
    m = cuts.moments(xv, bounds, flags=fv if with_flags else None, model=mv if with_model else None, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"
    S = len(bounds) - 1
    assert all(tuple(getattr(m, k).shape) == (D, S) for k in FIELDS) and m.hits.dtype == m.pairs.dtype == torch.int64 and m.mean.dtype == torch.float64
    got = host(m)
    want = ref.moments(x, bounds, flags=flags if with_flags else None, model=model if with_model else None)
    where = (D, T, seed, with_flags, with_model, padded)
    for k in ("hits", "pairs", "min", "max"):
        assert np.array_equal(got[k], want[k]), (k, where)
    nothing = want["hits"] == 0
    assert nothing[:, np.diff(bounds) == 0].all() and (not with_flags or T < 64 or nothing[D - 1, 1])
    for k in ref.NAMES:
        assert not got[k][nothing].any(), (k, where)
    worst = 0.0
    for k, b in ref.bounds_of(want).items():
        err = np.abs(got[k] - want[k])
        print(f"{where} {k}: max |got - ref| / bound = {(err / np.where(b > 0, b, 1)).max():.3g}")
        assert np.all(err <= b), (k, where)
        worst = max(worst, float((err / np.where(b > 0, b, 1)).max()))
    return worst


def test_the_bounds_of_the_cases_hold_every_length():
    used = set()
    for T in TIMES:
        for seed in range(3):
            used |= set(np.diff(make_bounds(T, seed)).tolist())
    assert used == set(LENGTHS)


@pytest.mark.parametrize("D", ROWS)
def test_moments_within_their_bounds_and_counts_exact(gpu_ctx, D):
    worst = 0.0
    for i, T in enumerate(TIMES):
        worst = max(worst, moments_case(gpu_ctx, D, T, i % 3, with_flags=True, with_model=i % 2 == 0, padded=i % 2 == 1))
        if T in (5, 257, 1025, 4099):
            worst = max(worst, moments_case(gpu_ctx, D, T, (i + 1) % 3, with_flags=False, with_model=i % 2 == 1, padded=i % 2 == 0))
    print(f"D {D}: max |got - ref| / bound = {worst:.3g}")


@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_exact_inputs_bit_for_bit(gpu_ctx, case):
    from maria_amd import cuts

    span, top, names, with_model = EXACT_CASES[case]
    bounds = power_of_two_bounds(top)
    for D in ROWS:
        x, model = exact_rows(D, int(bounds[-1]) + 2, span, 5 + D, with_model)
        want = ref.moments(x, bounds, model=model)
        for padded in (False, True):
            _, (xv, mv, _) = to_device(x, x if model is None else model, np.zeros(x.shape, np.uint8), padded)
            got = host(cuts.moments(xv, bounds, model=mv if with_model else None, ctx=gpu_ctx))
            assert np.array_equal(got["hits"], want["hits"]) and np.array_equal(got["pairs"], want["pairs"])
            for k in names:
                assert np.array_equal(bits(got[k]), bits(want[k])), (case, D, padded, k)


def test_sums_are_reproducible_alone_and_at_either_alignment(gpu_ctx):
    """The same bits on a second call, for a row alone, for a segment alone (its own two bounds), with other rows added,
    at either alignment, and whatever the flagged samples hold (the data, 1e30, NaN)."""
    import torch

    from maria_amd import cuts

    D, T = 33, 4099
    x, model, flags = rows(D, T, 8, exact=False)
    bounds = make_bounds(T, 1)
    S = len(bounds) - 1
    flags[7, :] = 1
    dx, dm, df = (torch.as_tensor(a).to(DEV) for a in (x, model, flags))
    first = host(cuts.moments(dx, bounds, flags=df, model=dm, ctx=gpu_ctx))
    assert np.isfinite(first["m4"]).all() and first["hits"][7].sum() == 0

    def same(got, sel, what):
        for k in FIELDS:
            assert np.array_equal(bits(first[k][sel]), bits(host(got)[k])), (what, k)

    same(cuts.moments(dx, bounds, flags=df, model=dm, ctx=gpu_ctx), np.s_[:], "again")
    for row in (0, 16, 32):
        same(cuts.moments(dx[row:row + 1], bounds, flags=df[row:row + 1], model=dm[row:row + 1], ctx=gpu_ctx), np.s_[row:row + 1], f"row {row}")
    for s in range(S):
        same(cuts.moments(dx, bounds[s:s + 2], flags=df, model=dm, ctx=gpu_ctx), np.s_[:, s:s + 1], f"segment {s}")
    more = [torch.cat([torch.roll(a, 5, 0), a]) for a in (dx, dm, df)]
    got = host(cuts.moments(more[0], bounds, flags=more[2], model=more[1], ctx=gpu_ctx))
    for k in FIELDS:
        assert np.array_equal(bits(first[k]), bits(got[k][D:])), ("other rows", k)
    for pitch, offset in ((4100, 0), (4101, 1), (4102, 3)):
        xv, mv, fv = (device_rows(v, pitch, offset, 0)[1] for v in (x, model, flags))
        same(cuts.moments(xv, bounds, flags=fv, model=mv, ctx=gpu_ctx), np.s_[:], (pitch, offset))
    for fill in (1e30, float("nan")):
        xx, mm = dx.clone(), dm.clone()
        xx[df != 0] = fill
        mm[df == 2] = -fill
        same(cuts.moments(xx, bounds, flags=df, model=mm, ctx=gpu_ctx), np.s_[:], fill)


def test_an_unflagged_nan_stays_in_its_segment(gpu_ctx):
    import torch

    from maria_amd import cuts

    D, T = 3, 1025
    x, model, flags = rows(D, T, 5, exact=False)
    bounds = make_bounds(T, 0)
    s = int(np.argmax(np.diff(bounds)))
    t = int(bounds[s]) + 70
    flags[1, t] = 0
    dx, df = torch.as_tensor(x).to(DEV), torch.as_tensor(flags).to(DEV)
    clean = host(cuts.moments(dx, bounds, flags=df, ctx=gpu_ctx))
    dx[1, t] = float("nan")
    got = host(cuts.moments(dx, bounds, flags=df, ctx=gpu_ctx))
    rest = np.ones(clean["mean"].shape, bool)
    rest[1, s] = False
    for k in ref.NAMES:
        assert np.isnan(got[k][1, s]), k
        assert np.array_equal(bits(got[k][rest]), bits(clean[k][rest])), k
    assert np.array_equal(got["hits"], clean["hits"]) and np.array_equal(got["pairs"], clean["pairs"])


def test_summarize_against_scipy(gpu_ctx):
    """``summarize`` of the device's moments against scipy.stats.skew / kurtosis, numpy's var and ptp on the kept samples.
    The bounds are the moments' bounds to first order: with r_k = bound(M_k) / M_k, var and std carry r_2 (std half of
    it), skew |skew| (r_3' + 1.5 r_2) with r_3' = bound(M_3) / |M_3|, kurtosis (kurtosis + 3) (r_4 + 2 r_2); scipy's own
    float64 evaluation (a two-pass mean and power sums of about n terms) is allowed n + 8 ulps of each value on top."""
    import torch
    from scipy import stats

    from maria_amd import cuts

    D, T = 3, 4099
    x, model, flags = rows(D, T, 12, exact=False)
    bounds = make_bounds(T, 2)
    dx, dm, df = (torch.as_tensor(a).to(DEV) for a in (x, model, flags))
    s = {k: v.cpu().numpy() for k, v in cuts.summarize(cuts.moments(dx, bounds, flags=df, model=dm, ctx=gpu_ctx), np.diff(bounds)).items()}
    want = ref.moments(x, bounds, flags=flags, model=model)
    b = ref.bounds_of(want)
    terms = x.astype(np.float64) - model.astype(np.float64)
    checked = 0
    for si, (lo, hi) in enumerate(ref.segments(bounds, T)):
        for d in range(D):
            keep = flags[d, lo:hi] == 0
            k = terms[d, lo:hi][keep]
            n = k.size
            assert s["hits"][d, si] == n and (hi <= lo or s["flagged_fraction"][d, si] == 1.0 - n / (hi - lo))
            if n == 0:
                assert all(np.isnan(s[name][d, si]) for name in ("mean", "var", "std", "skew", "kurtosis", "ptp", "min", "max", "sigma_diff"))
                continue
            assert s["ptp"][d, si] == np.ptp(k) and s["min"][d, si] == k.min() and s["max"][d, si] == k.max()
            if want["m2"][d, si] == 0:
                assert np.isnan(s["skew"][d, si]) and np.isnan(s["kurtosis"][d, si]) and s["var"][d, si] == 0
                continue
            own = (n + 8) * 2.0**-52
            r2, r4 = b["m2"][d, si] / want["m2"][d, si], b["m4"][d, si] / want["m4"][d, si]
            assert abs(s["var"][d, si] - k.var()) <= (r2 + own) * k.var() and abs(s["std"][d, si] - k.std()) <= (r2 / 2 + own) * k.std()
            sk, ku = stats.skew(k), stats.kurtosis(k)
            assert abs(s["skew"][d, si] - sk) <= b["m3"][d, si] / want["m2"][d, si] ** 1.5 * np.sqrt(n) + (1.5 * r2 + own) * abs(sk), (d, si)
            assert abs(s["kurtosis"][d, si] - ku) <= (r4 + 2 * r2 + own) * (ku + 3), (d, si)
            both = keep[1:] & keep[:-1]
            if both.any():
                white = np.sqrt(np.sum(np.diff(terms[d, lo:hi])[both] ** 2) / (2.0 * both.sum()))
                assert abs(s["sigma_diff"][d, si] - white) <= (b["d2"][d, si] / max(want["d2"][d, si], 1e-300) / 2 + own) * white
            checked += 1
    assert checked >= 3 * 10
    # white noise of sigma 1 on a strong linear drift: sigma_diff stays at the white level, std does not
    rng = np.random.default_rng(1)
    y = (rng.standard_normal((4, 4000)) + np.linspace(0.0, 40.0, 4000)).astype(np.float32)
    det = cuts.summarize(cuts.moments(torch.as_tensor(y).to(DEV), ctx=gpu_ctx))
    assert np.all(np.abs(det["sigma_diff"].cpu().numpy() - 1.0) < 0.05) and np.all(det["std"].cpu().numpy() > 10.0)


@pytest.mark.parametrize("value", [1, 2, 128])
def test_flag_segments_bit_for_bit(gpu_ctx, value):
    import torch

    from maria_amd import cuts

    for i, T in enumerate(TIMES):
        D = ROWS[(i + value) % 3]
        rng = np.random.default_rng(T + D + value)
        bounds = make_bounds(T, i % 3)
        S = len(bounds) - 1
        old = ((rng.random((D, T)) < 0.1) * rng.integers(1, 3, (D, T))).astype(np.uint8)
        mask = (rng.random((D, S)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (D, S)).astype(np.uint8)
        mask[D - 1] = 1
        want = ref.flag_segments(old, bounds, mask, value)
        covered = np.zeros(T, bool)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            covered[lo:hi] = True
        assert np.array_equal(want[:, ~covered], old[:, ~covered]) and (T < 3 or not covered[[0, -1]].any())
        # 16-byte accesses: pointer and pitch multiples of 16; bytes: the row pitch T, and T + 3 one byte in
        for pitch, offset in ((T + (-T) % 16, 0), (T, 0), (T + 3, 1)):
            for as_bool in (False, True):
                fbuf, fv = device_rows(old, pitch, offset, 9)
                d_mask = torch.as_tensor(mask).to(DEV)
                out = cuts.flag_segments(fv, bounds, d_mask != 0 if as_bool else d_mask, value=value, ctx=gpu_ctx)
                torch.cuda.synchronize()
                assert out is fv and np.array_equal(fv.cpu().numpy(), want), (T, D, pitch, offset, value)
                assert untouched_outside(fbuf, fv, 9), "written outside the rows"


def test_hostile_bounds_are_clamped(gpu_ctx):
    """The C entries with bounds below 0, above T and reversed: clamped, a reversed pair empty, nothing out of range."""
    import torch

    from maria_amd._lib import ptr

    D, T = 3, 300
    x, model, flags = rows(D, T, 21, exact=False)
    bufs, (xv, mv, fv) = to_device(x, model, flags, True)
    before = [b.clone() for b in bufs]
    raw = np.array([-2**31, -7, 5, 3, 3, 140, 120, T + 9, 2**31 - 1], np.int32)  # [0, 0) [0, 5) [5, 3) [3, 3) [3, 140) [140, 120) [120, 300) [300, 300)
    S = len(raw) - 1
    d_raw = torch.as_tensor(raw).to(DEV)
    stat = torch.full((D, S, 8), 7.0, dtype=torch.float64, device=DEV)
    count = torch.full((D, S, 2), 12345, dtype=torch.int32, device=DEV)
    gpu_ctx.call("mrx_tod_segment_moments", ptr(xv), T + 3, ptr(mv), T + 5, ptr(fv), T + 1, D, T, ptr(d_raw), S, ptr(stat), ptr(count))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"
    want = ref.moments(x, raw, flags=flags, model=model)
    got_stat, got_count = stat.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(got_count[..., 0], want["hits"]) and np.array_equal(got_count[..., 1], want["pairs"])
    assert want["hits"][:, [0, 2, 3, 5, 7]].sum() == 0 and want["hits"][:, [1, 4, 6]].all() and not got_stat[:, [0, 2, 3, 5, 7]].any() and not got_stat[..., 7].any()
    assert np.array_equal(got_stat[..., 4], want["min"]) and np.array_equal(got_stat[..., 5], want["max"])
    b = ref.bounds_of(want)
    for i, k in ((0, "mean"), (1, "m2"), (2, "m3"), (3, "m4"), (6, "d2")):
        assert np.all(np.abs(got_stat[..., i] - want[k]) <= b[k]), k
    # the flagging, bounds clamped at both ends (ascending: the reference's rule), then reversed ones: whichever segment
    # a sample is given to, nothing is written outside the rows, no flag is lost and only ``value`` is added
    asc = np.array([-2**31, -7, 5, 5, 140, T + 9, 2**31 - 1], np.int32)
    mask = np.array([[1, 1, 0, 1, 1, 1], [0, 0, 1, 0, 1, 1], [1, 0, 1, 1, 0, 1]], np.uint8)
    fbuf, fw = device_rows(flags, T + 7, 1, 9)
    d_asc, d_mask, d_ones = torch.as_tensor(asc).to(DEV), torch.as_tensor(mask).to(DEV), torch.ones((D, S), dtype=torch.uint8, device=DEV)
    gpu_ctx.call("mrx_tod_segment_flag", ptr(fw), T + 7, D, T, ptr(d_asc), 6, ptr(d_mask), 4)
    torch.cuda.synchronize()
    assert np.array_equal(fw.cpu().numpy(), ref.flag_segments(flags, asc, mask, 4)) and untouched_outside(fbuf, fw, 9)
    fbuf, fw = device_rows(flags, T + 7, 1, 9)
    gpu_ctx.call("mrx_tod_segment_flag", ptr(fw), T + 7, D, T, ptr(d_raw), S, ptr(d_ones), 4)
    torch.cuda.synchronize()
    got = fw.cpu().numpy()
    assert np.array_equal(got & ~np.uint8(4), flags) and (got & 4)[:, 5:120].all() and untouched_outside(fbuf, fw, 9)


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T, S = 4, 3000, 3
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    model = torch.zeros((D, T), dtype=torch.float32, device=DEV)
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    bound = torch.as_tensor(np.array([0, 1000, 1000, T], np.int32)).to(DEV)
    mask = torch.ones((D, S), dtype=torch.uint8, device=DEV)
    stat = torch.full((D, S, 8), 7.0, dtype=torch.float64, device=DEV)
    count = torch.full((D, S, 2), 12345, dtype=torch.int32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    mo = (ptr(x), T, ptr(model), T, ptr(flags), T, D, T, ptr(bound), S, ptr(stat), ptr(count))
    fl = (ptr(flags), T, D, T, ptr(bound), S, ptr(mask), 1)

    def put(args, *pairs):
        args = list(args)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    cases = {
        "mrx_tod_segment_moments": {
            "null x": put(mo, (0, None)), "null bound": put(mo, (8, None)), "null stat": put(mo, (10, None)), "null count": put(mo, (11, None)),
            "D 0": put(mo, (6, 0)), "T 0": put(mo, (7, 0)), "S 0": put(mo, (9, 0)), "S -1": put(mo, (9, -1)), "ld_x < T": put(mo, (1, T - 1)),
            "ld_m < T": put(mo, (3, T - 1)), "ld_f < T": put(mo, (5, T - 1)),
        },
        "mrx_tod_segment_flag": {
            "null flags": put(fl, (0, None)), "null bound": put(fl, (4, None)), "null mask": put(fl, (6, None)), "D 0": put(fl, (2, 0)),
            "T 0": put(fl, (3, 0)), "S 0": put(fl, (5, 0)), "ld_f < T": put(fl, (1, T - 1)), "value 0": put(fl, (7, 0)), "value 256": put(fl, (7, 256)),
            "value -1": put(fl, (7, -1)),
        },
    }
    for entry, bad in cases.items():
        for name, args in bad.items():
            assert getattr(lib, entry)(hd, *args) == -1, (entry, name)
            assert entry.encode() in lib.mrx_last_error(hd), (entry, name)
    torch.cuda.synchronize()
    assert bool((stat == 7.0).all()) and bool((count == 12345).all()) and not bool(flags.any()) and bool((x == 1.0).all())
    # a pitch of an array that is not given is not looked at
    assert lib.mrx_tod_segment_moments(hd, *put(mo, (2, None), (3, 0), (4, None), (5, 0))) == 0
    torch.cuda.synchronize()
    assert count[:, :, 0].tolist() == [[1000, 0, 2000]] * D and count[:, :, 1].tolist() == [[999, 0, 1999]] * D
    assert stat[:, :, 0].tolist() == [[1.0, 0.0, 1.0]] * D and not bool(stat[:, :, 1:4].any()) and not bool(stat[:, :, 6:].any())
    assert stat[:, :, 4].tolist() == [[1.0, 0.0, 1.0]] * D and stat[:, :, 5].tolist() == [[1.0, 0.0, 1.0]] * D
    mask[:, 2] = 0
    assert lib.mrx_tod_segment_flag(hd, *put(fl, (7, 255))) == 0
    torch.cuda.synchronize()
    assert bool((flags[:, :1000] == 255).all()) and not bool(flags[:, 1000:].any())


# ---- end to end: a simulated map + noise TOD with the fixture's defects ---------------------------------------------------

MAP = dict(n=128, width=1.0)


@pytest.fixture(scope="module")
def cut_fixture(gpu_ctx):
    """Simulation(map=a blob, noise=True) of 32 positions x 2 bands on a constant-elevation scan of 60 s at 50 Hz, K_RJ, and
    the same TOD with the defects of tests/test_host_cuts.py injected into its noise field; the reference's verdict on
    the dirty signal less the sampled sky, which must be the injected set with every criterion 1e-6 away from its
    threshold."""
    import torch

    from maria_amd import map as mmap
    from maria_amd import subscans
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import TOD, Plan, Simulation, sky_transform_stack
    from test_gpu_downsample import _centre

    bands = [Band(center=93e9, width=27e9, shape="top_hat", name="f093"), Band(center=150e9, width=41e9, shape="top_hat", name="f150")]
    n, width = MAP["n"], MAP["width"]
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    data = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0
    data = (data - data.mean()).astype(np.float32)
    dets = Detectors.hexagon(32, width / 2, bands, primary_size=30.0)
    dets.gamma = np.zeros(dets.n)  # polarised: the I weight is 0.5; an unpolarised detector's, 0.5 sqrt(2) sqrt(2), is 1 + 2^-52 in float64
    inst = Instrument(dets)
    site = Site(altitude=5000.0)
    plan = Plan.back_and_forth(start_time=1.7e9, duration=60.0, sample_rate=50.0, scan_center=(120.0, 55.0), throw=0.3, speed=0.5, accel=1.0)
    centre = _centre(plan.phi.astype(np.float32), plan.theta.astype(np.float32), sky_transform_stack(plan.time, site.latitude, site.longitude))
    sky = mmap.ProjectionMap(data, nu=150e9, width=width, center=np.degrees(centre), frame="ra/dec")
    (clean,) = Simulation(inst, plan, site, map=sky, noise=True, noise_seed=3, noise_kwargs={"correlated_noise_proportion": 0.0}).run()
    assert clean.units == "K_RJ" and set(clean.fields) == {"map", "noise"}
    fields = {k: np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, np.float32) for k, v in clean.data.items()}
    # every sample a multiple of one grain, 2^-26 of the power of two above the largest value the defects can reach: the
    # mappers' float64 sums of up to 2^20 such float32 samples are then exact in whatever order their atomics add, which
    # is what lets the map test below ask for the same bits (rounding moves a sample by 2^-27 of that power at most)
    grain = 2.0 ** (np.ceil(np.log2(32 * max(float(np.abs(v).max()) for v in fields.values()))) - 26)
    quantise = lambda a: (np.round(a.astype(np.float64) / grain) * grain).astype(np.float32)  # noqa: E731
    fields = {k: quantise(v) for k, v in fields.items()}
    assert fields["noise"].shape == (64, 3000) and np.array_equal(np.asarray(clean.dets.band_index), np.arange(64) // 32)
    bounds, _ = subscans.find_subscans(clean.coords._baz)
    assert len(bounds) - 1 >= 20
    noisy, touched = defects(fields["noise"], bounds)
    noisy = quantise(noisy)
    assert np.array_equal(noisy[~touched], fields["noise"][~touched]) and float(np.abs(noisy).max() + np.abs(fields["map"]).max()) < grain * 2.0**26
    assert all(np.array_equal(v.astype(np.float64) / grain, np.round(v.astype(np.float64) / grain)) for v in (noisy, *fields.values()))

    def tod(noise, flags=None):
        out = TOD({"map": torch.as_tensor(fields["map"]).to(DEV), "noise": torch.as_tensor(noise).to(DEV)}, clean.dets, clean.coords, units="K_RJ",
                  metadata=dict(clean.metadata), flags=flags)
        out._calibrator = getattr(clean, "_calibrator", None)
        return out

    groups = np.arange(64) // 32
    signal = (fields["map"] + noisy).astype(np.float32)  # the device's own float32 sum of the fields
    margins = []
    masks, cut, segs, new = reference_verdict(signal, bounds, None, groups, margins=margins, model=fields["map"])
    print(f"reference: cut {cut}, segments {segs}, least margin {min(margins):.3g}")
    assert cut == CUT_DETECTORS and segs == sorted(NOISY_SEGMENTS) and min(margins) >= 1e-6
    assert np.all(new[touched] != 0), "a defect is left unflagged"
    return dict(clean=tod(fields["noise"]), dirty=tod(noisy), make=tod, fields=fields, noisy=noisy, bounds=bounds, flags=new, masks=masks,
                centre=centre, bands=bands, groups=groups)


def test_cut_takes_exactly_the_injected_set(gpu_ctx, cut_fixture):
    import torch

    fx = cut_fixture
    dirty = fx["dirty"]
    kept = {k: v.clone() for k, v in dirty.data.items()}
    out = dirty.cut(model=dirty.data["map"], ctx=gpu_ctx)
    assert dirty.flags is None and "cuts" not in dirty.metadata and all(torch.equal(dirty.data[k], kept[k]) for k in kept)
    assert out.dets is dirty.dets and out.coords is dirty.coords and out.units == "K_RJ" and out._calibrator is dirty._calibrator
    assert out.fields == dirty.fields and all(torch.equal(out.data[k], kept[k]) and out.data[k] is not dirty.data[k] for k in kept)
    meta = out.metadata["cuts"]
    assert meta["cut_detectors"].tolist() == CUT_DETECTORS and sorted(map(tuple, meta["cut_segments"].tolist())) == sorted(NOISY_SEGMENTS)
    assert sorted(meta["masks"]) == sorted(fx["masks"]) and all(np.array_equal(meta["masks"][k], fx["masks"][k]) for k in fx["masks"])
    assert out.flags.dtype == torch.uint8 and np.array_equal(out.flags.cpu().numpy(), fx["flags"])
    assert meta["bounds"].tolist() == fx["bounds"].tolist() and meta["n_sigma"] == 5.0 and meta["n_sigma_segment"] == 5.0 and meta["value"] == 1
    assert meta["max_flagged"] == 0.5 and meta["max_bad_segments"] == 0.5 and meta["min_hits"] == 8 and meta["groups"].tolist() == fx["groups"].tolist()
    assert meta["criteria"] == ("white", "rms", "skew", "kurtosis", "flagged")
    assert meta["flagged_fraction_before"] == 0.0 and meta["flagged_fraction_after"] == float((fx["flags"] != 0).mean())
    # the clean TOD loses nothing
    none = fx["clean"].cut(model=fx["clean"].data["map"], ctx=gpu_ctx)
    assert none.metadata["cuts"]["cut_detectors"].size == 0 and none.metadata["cuts"]["cut_segments"].shape == (0, 2) and not bool(none.flags.any())


def test_maps_of_the_cut_tod_are_those_of_the_clean_one_with_its_flags(gpu_ctx, cut_fixture):
    """The defects lie wholly under the flags, and a flagged sample has no weight: BinMapper and the GLS map of the cut
    TOD equal, bit for bit, those of the clean TOD carrying the same flags; without the cut they differ.  The mappers add
    with float64 atomics in an order that is not fixed (include/mrx.h: "results agree with a serial sum to float64
    rounding"): on the TOD as simulated, two runs on the SAME input differed in 1290 of 15812 pixels by up to 2.3e-13
    relative, and cut against clean in 1375 by up to 3.8e-13, the same thing.  The fixture's samples are therefore
    multiples of one grain and its detectors' I weight a power of two, which makes every sum exact in any order.  The GLS map takes noise_weights="uniform": its
    default, 1 / var of the row, is taken over flagged samples too and differs between the two TODs by design."""
    from maria_amd.mappers import BinMapper, MaximumLikelihoodMapper

    fx = cut_fixture
    cut = fx["dirty"].cut(model=fx["dirty"].data["map"], ctx=gpu_ctx)
    free = fx["make"](fx["fields"]["noise"], flags=cut.flags)
    res = MAP["width"] / (MAP["n"] - 1)
    kw = dict(center=np.degrees(fx["centre"]), width=(MAP["n"] + 0.5) * res, resolution=res, stokes="I", nu=[b.center for b in fx["bands"]],
              frame="ra/dec", units="K_RJ")
    for cls, extra in ((BinMapper, {}), (MaximumLikelihoodMapper, {"noise_weights": "uniform"})):
        maps, full = {}, {}
        for name, tod in (("cut", cut), ("free", free), ("dirty", fx["dirty"])):
            mapper = cls([tod], **kw, **extra)
            maps[name] = np.asarray(mapper.run().data, np.float32)
            full[name] = np.asarray(mapper.products["data"], np.float64)
        hit = np.isfinite(full["free"])
        assert hit.mean() > 0.05 and np.array_equal(hit, np.isfinite(full["cut"]))
        print(f"{cls.__name__}: cut against clean with the same flags: {int((bits(full['cut']) != bits(full['free'])).sum())} of {int(hit.sum())} "
              f"float64 pixels differ; cut against dirty: {int((bits(full['dirty']) != bits(full['free'])).sum())}")
        assert np.array_equal(bits(maps["cut"]), bits(maps["free"])) and np.array_equal(bits(full["cut"]), bits(full["free"])), cls.__name__
        assert not np.array_equal(bits(maps["dirty"]), bits(maps["free"])), cls.__name__


def test_stats_and_cut_interfaces(gpu_ctx, cut_fixture):
    import torch

    from maria_amd import cuts

    fx = cut_fixture
    dirty, bounds, fields = fx["dirty"], fx["bounds"], fx["fields"]
    D, T = 64, 3000
    signal = (fields["map"] + fx["noisy"]).astype(np.float32)
    # stats: per segment and per detector against the reference, bounds in every form
    st = dirty.stats("subscans", model=fields["map"], ctx=gpu_ctx)  # a host model
    want_seg = ref.summarize(ref.moments(signal, bounds, model=fields["map"]))
    want_det = ref.summarize(ref.moments(signal, None, model=fields["map"]))
    assert st["bounds"].tolist() == bounds.tolist() and sorted(st["segments"]) == sorted(want_seg) == sorted(st["detectors"])
    for k in want_seg:
        assert tuple(st["segments"][k].shape) == (D, len(bounds) - 1) and tuple(st["detectors"][k].shape) == (D,)
        np.testing.assert_allclose(st["segments"][k].cpu().numpy(), want_seg[k], rtol=1e-9, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(st["detectors"][k].cpu().numpy(), want_det[k][:, 0], rtol=1e-9, atol=1e-12, err_msg=k)
    whole = dirty.stats(ctx=gpu_ctx)
    assert whole["bounds"].tolist() == [0, T] and tuple(whole["segments"]["std"].shape) == (D, 1)
    assert torch.equal(whole["segments"]["std"][:, 0], whole["detectors"]["std"])
    chunks = dirty.stats(700, ctx=gpu_ctx)
    assert chunks["bounds"].tolist() == [0, 700, 1400, 2100, 2800, 3000] and chunks["segments"]["hits"][0].tolist() == [700] * 4 + [200]
    own = dirty.stats(np.array([-5, 100, 100, 4000]), ctx=gpu_ctx)
    assert own["bounds"].tolist() == [0, 100, 100, 3000] and own["segments"]["hits"][3].tolist() == [100, 0, 2900]
    # a TOD that already has flags: kept, counted before and after, left out of the statistics; another value
    old = (np.random.default_rng(4).random((D, T)) < 0.02).astype(np.uint8) * 2
    old[12, :2000] = 2  # more than half flagged: cut by "flagged"
    flagged = fx["make"](fx["noisy"], flags=torch.as_tensor(old).to(DEV))
    out = flagged.cut(model=flagged.data["map"], value=8, ctx=gpu_ctx)
    masks, cut, segs, new = reference_verdict(signal, bounds, old, fx["groups"], model=fields["map"], value=8)
    assert cut == sorted(CUT_DETECTORS + [12]) and masks["flagged"][12] and segs == sorted(NOISY_SEGMENTS)
    meta = out.metadata["cuts"]
    assert meta["cut_detectors"].tolist() == cut and sorted(map(tuple, meta["cut_segments"].tolist())) == segs
    assert np.array_equal(out.flags.cpu().numpy(), new) and np.array_equal(flagged.flags.cpu().numpy(), old)
    assert np.array_equal(new & 2, old) and meta["flagged_fraction_before"] == float((old != 0).mean()) and meta["flagged_fraction_after"] == float((new != 0).mean())
    # bounds as an int and as an array; one group; fewer criteria; no segments; a lower share of bad segments
    for b in (250, np.arange(0, 3001, 250)):
        got = dirty.cut(bounds=b, groups=None, model=fields["map"], ctx=gpu_ctx).metadata["cuts"]
        masks, cut, segs, _ = reference_verdict(signal, np.arange(0, 3001, 250), None, None, model=fields["map"])
        assert got["bounds"].tolist() == list(range(0, 3001, 250)) and got["groups"] is None
        assert got["cut_detectors"].tolist() == cut and sorted(map(tuple, got["cut_segments"].tolist())) == segs
    got = dirty.cut(model=fields["map"], criteria=("kurtosis",), n_sigma_segment=None, ctx=gpu_ctx).metadata["cuts"]
    masks, cut, segs, _ = reference_verdict(signal, bounds, None, fx["groups"], model=fields["map"], criteria=("kurtosis",), n_sigma_segment=None)
    assert got["cut_detectors"].tolist() == cut and got["cut_segments"].shape == (0, 2) and sorted(got["masks"]) == ["kurtosis", "segments", "unusable"]
    got = dirty.cut(model=fields["map"], max_bad_segments=0.02, ctx=gpu_ctx).metadata["cuts"]
    assert got["cut_detectors"].tolist() == sorted(CUT_DETECTORS + [d for d, _ in NOISY_SEGMENTS]) and got["cut_segments"].shape == (0, 2)
    # without the model the sky stays in the statistics: still the reference's verdict on that signal
    got = dirty.cut(ctx=gpu_ctx).metadata["cuts"]
    masks, cut, segs, _ = reference_verdict(signal, bounds, None, fx["groups"])
    assert got["cut_detectors"].tolist() == cut and sorted(map(tuple, got["cut_segments"].tolist())) == segs
    # a downsampled TOD: the coordinates' own subscans, the dead and the noisy detector still cut
    low = dirty.downsample(2, ctx=gpu_ctx)
    cut_low = low.cut(model=low.data["map"], ctx=gpu_ctx)
    assert tuple(cut_low.flags.shape) == (D, 1500) and cut_low.metadata["downsample"]["factor"] == 2
    assert {NOISY, DEAD}.issubset(set(cut_low.metadata["cuts"]["cut_detectors"].tolist())) and cut_low.metadata["cuts"]["bounds"][-1] == 1500
    # refusals that need the fields
    for bad in (lambda: dirty.cut(groups=np.zeros(63, int)), lambda: dirty.cut(model=np.zeros((64, 2999), np.float32)),
                lambda: dirty.stats(model=np.zeros((63, 3000), np.float32))):
        with pytest.raises(ValueError):
            bad()
    assert cuts.CRITERIA == ("white", "rms", "skew", "kurtosis", "flagged")
