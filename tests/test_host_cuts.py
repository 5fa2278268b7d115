"""The host side of maria_amd.cuts without a GPU: the reference of tests/cuts_ref.py against numpy and scipy,
the inputs whose sums are exact in any order, the size of the mistakes the derived bounds see, ``find_outliers`` and
``decide`` against their numpy restatements, the cut fixture, and every Python-side refusal."""

import math

import cuts_ref as ref
import numpy as np
import pytest
from test_gpu_subscans import bits, make_bounds, rows

from maria_amd import cuts

def power_of_two_bounds(top):
    """[S + 1]: segments of 1, 2, 4 .. top samples side by side from sample 3 on."""
    return (3 + np.concatenate([[0], np.cumsum(2 ** np.arange(int(math.log2(top)) + 1))])).astype(np.int32)


def exact_rows(D, T, span, seed, with_model):
    rng = np.random.default_rng(seed)
    x = rng.integers(-span, span + 1, (D, T)).astype(np.float32)
    model = rng.integers(-span // 4, span // 4 + 1, (D, T)).astype(np.float32) if with_model else None
    return x, model


EXACT_CASES = {"all moments: integers in -4 .. 4, lengths <= 64": (4, 64, ref.NAMES, False),
               "mean, m2, d2: integers in -64 .. 64, lengths <= 1024": (64, 1024, ("mean", "m2", "min", "max", "d2"), True)}


@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_the_exact_inputs_are_exact_in_any_order(case):
    """The inputs of the device's bit-for-bit tests: fsum, forward and reversed naive summation give the same bits, so
    the reference does not depend on the order and any correct device order must reproduce it."""
    span, top, names, with_model = EXACT_CASES[case]
    bounds = power_of_two_bounds(top)
    x, model = exact_rows(3, int(bounds[-1]) + 2, span, 5, with_model)
    got = [ref.moments(x, bounds, model=model, total=t) for t in (math.fsum, ref.naive, lambda v: ref.naive(v, reverse=True))]
    assert np.array_equal(got[0]["hits"], np.broadcast_to(np.diff(bounds), got[0]["hits"].shape))
    for name in names:
        assert got[0][name].any()
        for other in got[1:]:
            assert np.array_equal(bits(got[0][name]), bits(other[name])), name


def test_reference_against_numpy_and_scipy():
    from scipy import stats

    rng = np.random.default_rng(1)
    D, T = 3, 700
    x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
    model = rng.standard_normal((D, T)).astype(np.float32)
    flags = ((rng.random((D, T)) < 0.1) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    bounds = np.array([-4, 10, 10, 300, 301, 650, 900])
    flags[2, 10:300] = 1  # one segment wholly flagged
    flags[0, 300] = 0
    m = ref.moments(x, bounds, flags=flags, model=model)
    s = ref.summarize(m)
    assert m["length"][0].tolist() == [10, 0, 290, 1, 349, 50]
    assert not any(m[k][:, 1].any() for k in ref.NAMES) and not any(m[k][2, 2] for k in ref.NAMES) and m["hits"][2, 2] == 0
    assert np.isnan(s["mean"][2, 2]) and np.isnan(s["sigma_diff"][2, 2]) and s["flagged_fraction"][2, 2] == 1.0 and np.isnan(s["flagged_fraction"][0, 1])
    for d, seg in ((0, 2), (1, 4), (2, 5), (0, 0)):
        lo, hi = ref.segments(bounds, T)[seg]
        keep = flags[d, lo:hi] == 0
        t = (x[d, lo:hi].astype(np.float64) - model[d, lo:hi])
        k = t[keep]
        assert m["hits"][d, seg] == keep.sum() and m["pairs"][d, seg] == (keep[1:] & keep[:-1]).sum()
        np.testing.assert_allclose(s["mean"][d, seg], k.mean(), rtol=1e-13)
        np.testing.assert_allclose(s["var"][d, seg], k.var(), rtol=1e-12)
        np.testing.assert_allclose(s["skew"][d, seg], stats.skew(k), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(s["kurtosis"][d, seg], stats.kurtosis(k), rtol=1e-10, atol=1e-12)
        assert s["ptp"][d, seg] == np.ptp(k) and s["min"][d, seg] == k.min() and s["max"][d, seg] == k.max()
        both = keep[1:] & keep[:-1]
        np.testing.assert_allclose(m["d2"][d, seg], np.sum(np.diff(t)[both] ** 2), rtol=1e-13)
        assert s["flagged_fraction"][d, seg] == 1.0 - keep.sum() / (hi - lo)
    # the one-sample segment: everything is that sample, no spread, no pair
    assert m["hits"][0, 3] == 1 and m["m2"][0, 3] == 0 and np.isnan(s["skew"][0, 3]) and np.isnan(s["sigma_diff"][0, 3]) and s["std"][0, 3] == 0
    # an unflagged NaN makes its own (row, segment) NaN and nothing else
    x[1, 20] = np.nan
    flags[1, 20] = 0
    m2 = ref.moments(x, bounds, flags=flags, model=model)
    for name in ref.NAMES:
        assert np.isnan(m2[name][1, 2]), name
        rest = np.ones((D, 6), bool)
        rest[1, 2] = False
        assert np.array_equal(bits(m2[name][rest]), bits(m[name][rest])), name


def test_the_bounds_see_the_usual_mistakes():
    """On the Gaussian rows of the device tests, float32 accumulation, a mean rounded to float32 and one dropped sample
    each leave the derived bounds by a wide margin on every segment of 63 samples or more; a different float64 order
    (naive forward summation) stays inside them.  The float32 mean shows in m3 and m4; m2 is blind to any error of the mean
    to first order (it changes by n dmu^2 only, the sum of e being zero), which is why it is least at the true mean."""
    D, T = 3, 4099
    x, model, flags = rows(D, T, 11, exact=False)
    bounds = make_bounds(T, 7)
    m = ref.moments(x, bounds, flags=flags, model=model)
    b = ref.bounds_of(m)
    long = m["length"] >= 63
    assert long.sum() >= 3 * 8
    forward = ref.moments(x, bounds, flags=flags, model=model, total=ref.naive)
    for name in b:
        assert np.all(np.abs(forward[name] - m[name]) <= b[name]), name

    def f32_sum(v):
        s = np.float32(0.0)
        for a in v:
            s = np.float32(s + np.float32(a))
        return float(s)

    single = ref.moments(x, bounds, flags=flags, model=model, total=f32_sum)
    for name in b:
        assert np.all(np.abs(single[name] - m[name])[long] > 100 * b[name][long]), name
    # the mean rounded to float32, the sums in float64: the central sums feel it (d2 and the mean's own error do not count)
    terms = x.astype(np.float64) - model.astype(np.float64)
    dropped = flags.copy()
    worst = {k: np.inf for k in ("m2", "m3", "m4")}
    for s, (lo, hi) in enumerate(ref.segments(bounds, T)):
        if hi - lo < 63:
            continue
        for d in range(D):
            kept = terms[d, lo:hi][flags[d, lo:hi] == 0]
            e = kept - float(np.float32(m["mean"][d, s]))
            e2 = e * e
            for k, v in (("m2", e2), ("m3", e2 * e), ("m4", e2 * e2)):
                worst[k] = min(worst[k], abs(math.fsum(v) - m[k][d, s]) / b[k][d, s])
            dropped[d, lo + int(np.flatnonzero(flags[d, lo:hi] == 0)[3])] = 1
    assert worst["m3"] > 10 and worst["m4"] > 10, worst
    less = ref.moments(x, bounds, flags=dropped, model=model)
    for name in b:
        assert np.all(np.abs(less[name] - m[name])[long] > 1e6 * b[name][long]), name


def np_outliers(v, groups, n_sigma, side, eligible):
    """find_outliers restated with numpy, entry by entry."""
    v = np.asarray(v)
    out, unusable = np.zeros(v.shape, bool), np.zeros(v.shape, bool)
    for i in range(v.size):
        if groups[i] < 0:
            continue
        if not (eligible[i] and np.isfinite(v[i])):
            unusable[i] = True
            continue
        mates = [j for j in range(v.size) if groups[j] == groups[i] and eligible[j] and np.isfinite(v[j])]
        med = np.median(v[mates])
        scale = 1.4826 * np.median(np.abs(v[mates] - med))
        far = {"both": abs(v[i] - med), "high": v[i] - med, "low": med - v[i]}[side]
        out[i] = scale > 0 and far > n_sigma * scale
    return out, unusable


@pytest.mark.parametrize("side", cuts.SIDES)
def test_find_outliers_against_numpy(side):
    import torch

    rng = np.random.default_rng(3)
    n = 120
    v = rng.standard_normal(n)
    groups = rng.permutation(np.repeat([0, 1, 2, 4, 5, -1], n // 6))  # random row order; group 3 is empty; -1 is left out
    v[groups == 1] = 2.5  # scale == 0: nothing is an outlier, whatever else holds
    v[np.flatnonzero(groups == 1)[0]] = 9.0
    v[np.flatnonzero(groups == 5)[:2]] = 1.0  # an even count with ties
    for g, val in ((0, 40.0), (0, -35.0), (2, -60.0), (4, 7.5), (4, np.nan), (2, np.inf), (0, -np.inf), (-1, 99.0)):
        v[rng.choice(np.flatnonzero(groups == g))] = val
    eligible = rng.random(n) > 0.1
    for elig in (None, eligible):
        for n_sigma in (3.0, 5.0):
            got = cuts.find_outliers(torch.as_tensor(v), groups, n_sigma, side, None if elig is None else torch.as_tensor(elig))
            want = np_outliers(v, groups, n_sigma, side, np.ones(n, bool) if elig is None else elig)
            again = ref.find_outliers(v, groups, n_sigma, side, elig)
            for a, w, r in zip(got, want, again):
                assert a.dtype == torch.bool and np.array_equal(a.numpy(), w) and np.array_equal(r, w), (side, n_sigma)
            assert not got[0].numpy()[groups == 1].any() and not got[0].numpy()[groups == -1].any() and not (got[0] & got[1]).any()
    assert want[0].sum() >= 1 and want[1].sum() >= 3
    # two dimensions, one group a row, as the segments use it; None: one group; everything ineligible
    v2 = rng.standard_normal((7, 13))
    v2[2, 5] = 30.0
    r2 = np.broadcast_to(np.arange(7)[:, None], v2.shape)
    got = cuts.find_outliers(torch.as_tensor(v2), torch.as_tensor(r2.copy()), 5.0, side)
    want = np_outliers(v2.reshape(-1), r2.reshape(-1), 5.0, side, np.ones(v2.size, bool))
    assert np.array_equal(got[0].numpy().reshape(-1), want[0]) and got[0].numpy()[2, 5] == (side != "low")
    one = cuts.find_outliers(torch.as_tensor(v2[2]), None, 5.0, side)
    assert one[0].numpy()[5] == (side != "low") and not one[1].any()
    none = cuts.find_outliers(torch.as_tensor(v2[2]), None, 5.0, side, torch.zeros(13, dtype=torch.bool))
    assert not none[0].any() and none[1].all()
    for bad in (lambda: cuts.find_outliers(torch.as_tensor(v2[2]).float(), None, 5.0), lambda: cuts.find_outliers(v2[2], None, 5.0),
                lambda: cuts.find_outliers(torch.as_tensor(v2[2]), None, 0.0), lambda: cuts.find_outliers(torch.as_tensor(v2[2]), None, 5.0, "up"),
                lambda: cuts.find_outliers(torch.as_tensor(v2[2]), np.zeros(12, int), 5.0), lambda: cuts.find_outliers(torch.as_tensor(v2[2]), np.full(13, -2), 5.0),
                lambda: cuts.find_outliers(torch.as_tensor(v2[2]), np.zeros(13), 5.0),
                lambda: cuts.find_outliers(torch.as_tensor(v2[2]), None, 5.0, eligible=torch.ones(13))):
        with pytest.raises(ValueError):
            bad()


# ---- the cut fixture: what the end-to-end tests inject and what must be cut ------------------------------------------------

NOISY, SPIKY, DEAD, MOSTLY = 5, 38, 17, 50       # detectors (of 64: 32 positions x 2 bands, band = detector // 32)
NOISY_SEGMENTS = [(9, 3), (44, 7)]               # (detector, segment)
CUT_DETECTORS = sorted([NOISY, SPIKY, DEAD, MOSTLY])


def defects(data, bounds, seed=2):
    """``inject_bad`` with the fixture's defects: (bad data, touched); MOSTLY gets all but three of its segments noisy."""
    S = len(bounds) - 1
    mostly = [(MOSTLY, s) for s in range(S) if s not in (1, S // 2, S - 2)]
    return cuts.inject_bad(data, bounds, noisy=[NOISY], spiky=[SPIKY], dead=[DEAD], noisy_segments=NOISY_SEGMENTS + mostly, seed=seed)


def reference_verdict(signal, bounds, flags, groups, margins=None, model=None, value=1, n_sigma_segment=5.0, **kw):
    """(masks, cut detectors, bad segments outside them, the flags) of TOD.cut by the reference alone: the segments first,
    the detectors with the bad segments flagged."""
    flags = np.zeros(np.shape(signal), np.uint8) if flags is None else flags
    seg = ref.summarize(ref.moments(signal, bounds, flags=flags, model=model))
    bad = ref.bad_segments(seg, groups, n_sigma_segment, kw.get("min_hits", 8), margins)
    new = ref.flag_segments(flags, bounds, bad, value)
    det = ref.summarize(ref.moments(signal, None, flags=new, model=model))
    masks, cut = ref.decide(det, seg, bad, groups, margins=margins, **kw)
    new[cut] |= np.uint8(value)
    return masks, np.flatnonzero(cut).tolist(), sorted(map(tuple, np.argwhere(bad & ~cut[:, None]).tolist())), new


def host_fixture():
    """A stand-in for the simulated TOD of tests/test_gpu_cuts.py made on the host: 64 detectors in two bands of different
    white levels over 3000 samples in 13 subscans, white noise plus a slow drift, and old flags at 2 %."""
    from test_host_subscans import scan_azimuth

    from maria_amd import subscans

    rng = np.random.default_rng(8)
    D, T = 64, 3000
    bounds, _ = subscans.find_subscans(scan_azimuth()[1])
    level = np.where(np.arange(D) < 32, 1.0, 2.5)[:, None] * rng.uniform(0.9, 1.1, (D, 1))
    clean = (level * rng.standard_normal((D, T)) + 3.0 * np.sin(np.arange(T) / 400.0 + rng.uniform(0, 6, (D, 1)))).astype(np.float32)
    flags = (rng.random((D, T)) < 0.02).astype(np.uint8) * 2
    return clean, bounds, flags, np.arange(D) // 32


def test_the_reference_cuts_the_injected_set_with_a_margin():
    clean, bounds, flags, groups = host_fixture()
    assert len(bounds) - 1 == 13
    bad, touched = defects(clean, bounds)
    assert np.array_equal(bad[~touched], clean[~touched]) and touched[[NOISY, DEAD, MOSTLY]].any(axis=1).all() and 0.01 < touched[SPIKY].mean() < 0.03
    assert not touched[[d for d in range(64) if d not in CUT_DETECTORS + [d for d, _ in NOISY_SEGMENTS]]].any()
    masks, cut, segs, new = reference_verdict(clean, bounds, flags, groups)
    assert cut == [] and segs == [] and np.array_equal(new, flags), "the clean fixture is cut"
    margins = []
    masks, cut, segs, new = reference_verdict(bad, bounds, flags, groups, margins=margins)
    assert cut == CUT_DETECTORS and segs == sorted(NOISY_SEGMENTS)
    assert masks["white"][[NOISY, DEAD, MOSTLY]].all() and masks["kurtosis"][SPIKY] and not masks["flagged"].any() and not masks["unusable"].any()
    assert len(margins) > 64 * 4 and min(margins) >= 1e-6, min(margins)
    assert np.all(new[touched] != 0), "a defect is left unflagged"
    # the rules through maria_amd.cuts on host tensors give the reference's masks
    import torch

    as_t = lambda s: {k: torch.as_tensor(v) for k, v in s.items()}  # noqa: E731

    def both(signal, f, g, **kw):
        seg = ref.summarize(ref.moments(signal, bounds, flags=f))
        want_bad = ref.bad_segments(seg, g, kw.get("n_sigma_segment", 5.0))
        got_bad = cuts.bad_segments(as_t(seg), g, kw.pop("n_sigma_segment", 5.0))
        assert np.array_equal(got_bad.numpy(), want_bad)
        det = ref.summarize(ref.moments(signal, None, flags=ref.flag_segments(f, bounds, want_bad, 1)))
        want_masks, want_cut = ref.decide(det, seg, want_bad, g, **kw)
        got_masks, got_cut = cuts.decide(as_t(det), as_t(seg), got_bad, g, **kw)
        assert sorted(got_masks) == sorted(want_masks) and all(np.array_equal(got_masks[k].numpy(), want_masks[k]) for k in want_masks)
        assert np.array_equal(got_cut.numpy(), want_cut)
        return want_masks, np.flatnonzero(want_cut).tolist(), want_bad

    _, cut, got_bad = both(bad, flags, groups)
    assert cut == CUT_DETECTORS and sorted(map(tuple, np.argwhere(got_bad[[d for d, _ in NOISY_SEGMENTS]]).tolist())) == [(0, 3), (1, 7)]
    # a lower share of bad segments cuts the detectors with one noisy segment whole; a wholly flagged and a constant detector
    # are unusable; "flagged" above its threshold; a detector outside every group is judged by nothing
    _, cut, _ = both(bad, flags, groups, max_bad_segments=0.05)
    assert cut == sorted(CUT_DETECTORS + [d for d, _ in NOISY_SEGMENTS])
    f2, b2, g2 = flags.copy(), bad.copy(), groups.copy()
    f2[3] = 1
    f2[20, :1800] = 1
    b2[30] = 4.0
    g2[NOISY] = -1
    masks, cut, _ = both(b2, f2, g2)
    assert cut == sorted([3, 20, 30, SPIKY, DEAD, MOSTLY])
    assert masks["unusable"][[3, 30]].all() and masks["flagged"][[3, 20]].all() and masks["unusable"].sum() == 2
    masks, cut, none = both(b2, f2, g2, criteria=("flagged",), n_sigma_segment=None)
    assert cut == [3, 20] and not none.any() and sorted(masks) == ["flagged", "segments", "unusable"]


def test_summarize_on_host_tensors_is_the_reference():
    import torch

    x, model, flags = rows(3, 1025, 4, exact=False)
    bounds = make_bounds(1025, 2)
    flags[2, bounds[1]:bounds[2]] = 1
    m = ref.moments(x, bounds, flags=flags, model=model)
    want = ref.summarize(m)
    t = lambda k: torch.as_tensor(m[k])  # noqa: E731
    got = cuts.summarize(cuts.Moments(t("hits"), t("pairs"), *(t(k) for k in ref.NAMES)), np.diff(bounds))
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=4e-16, atol=0, equal_nan=True, err_msg=k)
    assert "flagged_fraction" not in cuts.summarize(cuts.Moments(t("hits"), t("pairs"), *(t(k) for k in ref.NAMES)))
    with pytest.raises(ValueError):
        cuts.summarize(cuts.Moments(t("hits"), t("pairs"), *(t(k) for k in ref.NAMES)), [1, 2])


def test_chunk_bounds_and_inject_bad():
    assert cuts.chunk_bounds(10, 4).tolist() == [0, 4, 8, 10] and cuts.chunk_bounds(8, 4).tolist() == [0, 4, 8] and cuts.chunk_bounds(3, 5).tolist() == [0, 3]
    assert cuts.chunk_bounds(1, 1).tolist() == [0, 1] and cuts.chunk_bounds(10, 4).dtype == np.int32
    for bad in (lambda: cuts.chunk_bounds(0, 4), lambda: cuts.chunk_bounds(10, 0), lambda: cuts.chunk_bounds(10, 2.5), lambda: cuts.chunk_bounds(2**31, 4)):
        with pytest.raises(ValueError):
            bad()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((6, 500)).astype(np.float32)
    bounds = [0, 100, 250, 500]
    out, touched = cuts.inject_bad(x, bounds, noisy=[0], spiky=[1], dead=[2], noisy_segments=[(3, 1)], seed=1)
    again, _ = cuts.inject_bad(x, bounds, noisy=[0], spiky=[1], dead=[2], noisy_segments=[(3, 1)], seed=1)
    assert out.dtype == np.float32 and np.array_equal(out, again) and out is not x and np.array_equal(out[4:], x[4:])
    white = lambda a: np.sqrt(np.mean(np.diff(a.astype(np.float64)) ** 2) / 2)  # noqa: E731
    assert 5 < white(out[0]) / white(x[0]) < 7.5 and white(out[2]) < 2e-3 * white(x[2]) and abs(out[2].mean() - x[2].mean()) < 1e-3
    assert touched[3].tolist() == [False] * 100 + [True] * 150 + [False] * 250 and np.array_equal(out[3, ~touched[3]], x[3, ~touched[3]])
    assert 5 < white(out[3, 100:250]) / white(x[3, 100:250]) < 8 and np.abs(out[1] - x[1])[touched[1]].min() > 10 * white(x[1])
    for bad in (lambda: cuts.inject_bad(x, bounds, noisy=[6], seed=1), lambda: cuts.inject_bad(x, bounds, noisy_segments=[(0, 3)], seed=1),
                lambda: cuts.inject_bad(x[0], bounds, seed=1), lambda: cuts.inject_bad(x, [0, 300, 200], seed=1), lambda: cuts.inject_bad(x, [5], seed=1)):
        with pytest.raises(ValueError):
            bad()


def test_python_refusals_come_before_any_device_call():
    """Host tensors: every refusal of the C entries, and bounds that do not ascend, raise ValueError in Python, and a valid
    call raises at the last check, "must be a device tensor", without touching a device."""
    import torch

    D, T, S = 4, 32, 3
    x = torch.zeros((D, T), dtype=torch.float32)
    flags = torch.zeros((D, T), dtype=torch.uint8)
    mask = torch.ones((D, S), dtype=torch.bool)
    bounds = np.array([0, 10, 20, 32], np.int32)
    last = "must be a device tensor"
    for good in (lambda: cuts.moments(x), lambda: cuts.moments(x, bounds, flags=flags, model=x), lambda: cuts.moments(x, [-3, 5, 5, 40]),
                 lambda: cuts.flag_segments(flags, bounds, mask), lambda: cuts.flag_segments(flags, torch.as_tensor(bounds), mask.to(torch.uint8), value=255)):
        with pytest.raises(ValueError, match=last):
            good()
    mo, fs = cuts.moments, cuts.flag_segments
    bad = [
        lambda: mo(x.double()), lambda: mo(x[:0]), lambda: mo(x[:, ::2]), lambda: mo(x, bounds[:1]), lambda: mo(x, bounds[None]),
        lambda: mo(x, bounds.astype(np.float64)), lambda: mo(x, bounds[::-1].copy()), lambda: mo(x, np.array([0, 2**31])),
        lambda: mo(x, bounds, flags=flags[:, :5]), lambda: mo(x, bounds, flags=flags.float()), lambda: mo(x, bounds, model=x[:2]),
        lambda: mo(x, bounds, model=x.double()), lambda: fs(flags.float(), bounds, mask), lambda: fs(flags[0], bounds, mask), lambda: fs(flags[:, ::2], bounds, mask[:, :1]),
        lambda: fs(flags, bounds[::-1].copy(), mask), lambda: fs(flags, bounds, mask[:, :2]), lambda: fs(flags, bounds, mask[:3]), lambda: fs(flags, bounds, mask.float()),
        lambda: fs(flags, bounds, mask.numpy()), lambda: fs(flags, bounds, mask, value=0), lambda: fs(flags, bounds, mask, value=256), lambda: fs(flags, bounds, mask, value=1.5),
        lambda: fs(flags, bounds, mask, value=True), lambda: fs(flags[:0], bounds, mask[:0]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError) as err:
            call()
        assert last not in str(err.value), f"refusal {i} got as far as the device check"


def test_tod_method_refusals():
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    T = 16
    coords = Coordinates(np.arange(T) / 10.0, np.linspace(0, 1, T), np.full(T, 1.0))
    dets = Detectors(np.zeros((3, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(3, int))
    tod = TOD({"a": np.zeros((3, T), np.float32)}, dets=dets, coords=coords)
    assert tod._segment_bounds(None).tolist() == [0, 16] and tod._segment_bounds(5).tolist() == [0, 5, 10, 15, 16]
    assert tod._segment_bounds([-3, 4, 40]).tolist() == [0, 4, 16] and tod._segment_bounds("subscans").tolist() == [0, 16]
    for bad in (lambda: tod.cut(bounds=[0, 9, 4, 16]), lambda: tod.cut(bounds=[0]), lambda: tod.cut(bounds=[0.0, 16.0]), lambda: tod.cut(bounds="scans"),
                lambda: tod.cut(bounds=0), lambda: tod.cut(groups="array"), lambda: tod.cut(groups=[0, 0, -2]), lambda: tod.cut(groups=[[0, 0, 0]]),
                lambda: tod.cut(groups=[0.0, 0.0, 0.0]), lambda: tod.cut(n_sigma=0), lambda: tod.cut(n_sigma_segment=-1.0), lambda: tod.cut(max_flagged=1.5),
                lambda: tod.cut(max_bad_segments=-0.1), lambda: tod.cut(min_hits=-1), lambda: tod.cut(min_hits=2.5), lambda: tod.cut(criteria=()),
                lambda: tod.cut(criteria=("white", "knee")), lambda: tod.cut(value=0), lambda: tod.cut(value=256), lambda: tod.cut(value=1.5),
                lambda: tod.stats(bounds=[0, 9, 4, 16]), lambda: tod.stats(bounds="scans"), lambda: tod.stats(bounds=2.5)):
        with pytest.raises(ValueError):
            bad()
