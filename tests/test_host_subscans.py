"""The host side of maria_amd.subscans without a GPU: the constant-elevation scan against its piecewise
formula, the segmentation, every Python-side refusal, and the reference of tests/subscans_ref.py against numpy's Legendre
series and a least-squares fit."""

import numpy as np
import pytest
import subscans_ref as ref

from maria_amd import subscans

# the front-end scan of test_gpu_subscans.py: 13 segments, the last of 25 samples (13 once the turnarounds are flagged)
SCAN = dict(duration=60.0, sample_rate=50.0, throw=2.0, speed=1.0, accel=2.0)


def scan_azimuth(centre=120.0, **kw):
    kw = {**SCAN, **kw}
    t = np.arange(0.0, kw["duration"], 1.0 / kw["sample_rate"])
    return t, np.radians(centre + subscans.back_and_forth(t, kw["throw"], kw["speed"], kw["accel"]))


def test_back_and_forth_against_its_piecewise_formula():
    throw, speed, accel = 2.0, 1.0, 2.0
    tc, tt = 2 * throw / speed, 2 * speed / accel
    period = 2 * (tc + tt)
    t = np.linspace(0.0, 3 * period, 30001)
    x = subscans.back_and_forth(t, throw, speed, accel)
    assert x[0] == -throw and x[1] > x[0]  # starts at -throw moving up
    np.testing.assert_allclose(subscans.back_and_forth(t + period, throw, speed, accel), x, atol=1e-12)  # periodic
    np.testing.assert_allclose(subscans.back_and_forth(t + period / 2, throw, speed, accel), -x, atol=1e-12)
    over = speed**2 / (2 * accel)
    assert abs(x.max() - (throw + over)) <= 1e-6 and abs(x.min() + (throw + over)) <= 1e-6
    assert subscans.back_and_forth(tc + tt / 2, throw, speed, accel) == throw + over  # the apex itself
    # by hand, second by second through the first half period: the crossing, then the parabola
    for tau, want in ((0.0, -2.0), (1.0, -1.0), (3.5, 1.5), (4.0, 2.0), (4.25, 2.0 + 0.25 - 0.0625), (4.5, 2.25), (5.0, 2.0), (6.0, 1.0), (9.5, -2.25)):
        assert abs(float(subscans.back_and_forth(tau, throw, speed, accel)) - want) <= 1e-12, tau
    # |velocity| = speed outside the turnarounds, below it inside, continuous everywhere
    v = np.diff(x) / np.diff(t)
    mid = (t[:-1] + t[1:]) / 2 % (tc + tt)
    crossing = mid < tc - 1e-3
    np.testing.assert_allclose(np.abs(v[crossing]), speed, rtol=1e-9)
    turning = (mid > tc + 1e-3) & (mid < tc + tt - 1e-3)
    assert np.all(np.abs(v[turning]) < speed)
    assert np.abs(np.diff(v)).max() <= 1.01 * accel * (t[1] - t[0])
    for bad in ((0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, 0.0), (1.0, -1.0, 1.0), (np.inf, 1.0, 1.0)):
        with pytest.raises(ValueError):
            subscans.back_and_forth(t, *bad)


def test_plan_back_and_forth():
    from maria_amd.sim import Plan

    plan = Plan.back_and_forth(start_time=1.7e9, scan_center=(120.0, 55.0), **SCAN)
    t, az = scan_azimuth()
    assert plan.time.shape == (3000,) and plan.time[0] == 1.7e9 and plan.frame == "az/el"
    assert np.array_equal(plan.phi, np.radians(120.0 + subscans.back_and_forth(plan.time - 1.7e9, 2.0, 1.0, 2.0)))
    # numpy's arange at 1.7e9 drifts by up to 6e-5 s over the 3000 samples: 6e-5 degrees of azimuth at 1 degree / s
    np.testing.assert_allclose(plan.phi, az, rtol=0, atol=np.radians(1e-4))
    assert np.all(plan.theta == np.radians(55.0))


def test_find_subscans_on_the_scan():
    t, az = scan_azimuth()
    bounds, turn = subscans.find_subscans(az)
    assert bounds.dtype == np.int32 and turn.dtype == np.uint8 and turn.shape == (3000,)
    assert bounds.tolist() == [0] + list(range(225, 3000, 250)) + [3000]  # the apexes at 4.5 s + 5 s k
    assert len(bounds) - 1 == 13 and bounds[-1] - bounds[-2] == 25
    assert abs(turn.mean() - 0.18) <= 0.01  # |v| < 0.9 speed during 0.9 s of every 5 s
    assert int((turn[bounds[-2]:] == 0).sum()) < 4  # under-determined at order 3 once the turnarounds are flagged
    # each segment is monotonic, and neighbours move in opposite directions
    d = [np.sign(np.diff(az[lo:hi + 1])) for lo, hi in zip(bounds[:-1], bounds[1:])]
    assert all(len(set(s.tolist())) == 1 for s in d) and all(a[0] != b[0] for a, b in zip(d[:-1], d[1:]))
    # through a wrap at 2 pi, and from the other end of the throw
    for centre in (359.0, 0.5):
        b2, t2 = subscans.find_subscans(np.radians(centre + subscans.back_and_forth(t, 2.0, 1.0, 2.0)) % (2 * np.pi))
        v = np.abs(np.diff(az))  # the wrap's rounding may move a sample that sits on the threshold itself, and no other
        on_the_threshold = np.append(np.abs(v / np.median(v) - 0.9) < 1e-9, True)
        assert b2.tolist() == bounds.tolist() and np.array_equal(t2[~on_the_threshold], turn[~on_the_threshold])
    # turn_frac 0: no turnaround; bad values
    assert not subscans.find_subscans(az, turn_frac=0.0)[1].any()
    for bad in (lambda: subscans.find_subscans(az, turn_frac=-0.1), lambda: subscans.find_subscans(az, turn_frac=1.5),
                lambda: subscans.find_subscans(az[None]), lambda: subscans.find_subscans(az[:0]), lambda: subscans.find_subscans(np.array([0.0, np.nan]))):
        with pytest.raises(ValueError):
            bad()


def test_find_subscans_flat_stretches_and_short_rows():
    # zeros take the sign before them, leading zeros the first nonzero sign
    az = np.array([1.0, 1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 2.0, 1.0, 1.0, 2.0, 2.0])
    #         v =   0    0    +    +    0    0    -    -    0    +    0    0(rep)
    bounds, turn = subscans.find_subscans(az, turn_frac=0.9)
    assert bounds.tolist() == [0, 6, 9, 12]
    assert not turn.any()  # median |v| = 0: nothing is below it
    bounds, turn = subscans.find_subscans(np.array([0.0, 1.0, 2.0, 2.0, 3.0, 4.0, 4.1, 3.0, 2.0, 1.0]))
    #                                        v =     +    +    0    +    +   .1  -1.1   -    -    -(rep)
    assert bounds.tolist() == [0, 6, 10] and turn.tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0, 0]  # median |v| = 1
    assert [b.tolist() for b in subscans.find_subscans(np.array([0.3]))] == [[0, 1], [0]]
    assert [b.tolist() for b in subscans.find_subscans(np.array([0.3, 0.4]))] == [[0, 2], [0, 0]]
    assert [b.tolist() for b in subscans.find_subscans(np.array([0.3, 0.3]))] == [[0, 2], [0, 0]]
    assert [b.tolist() for b in subscans.find_subscans(np.full(50, 1.0))] == [[0, 50], [0] * 50]
    assert subscans.find_subscans(np.array([0.0, 1.0, 0.0]))[0].tolist() == [0, 1, 3]


def test_reference_basis_against_numpy_legendre():
    from numpy.polynomial import legendre

    worst = 0.0
    for L in (1, 2, 3, 5, 64, 257, 2049):
        P = ref.basis(L, 8)
        u = np.linspace(-1.0, 1.0, L) if L > 1 else np.zeros(1)
        for n in range(8):
            want = legendre.legval(u, np.eye(8)[n])
            worst = max(worst, float(np.abs(P[n] - want).max()))
    assert worst <= 1e-14, worst
    assert ref.basis(1, 3).tolist() == [[1.0], [0.0], [-0.5]] and ref.basis(2, 2).tolist() == [[1.0, 1.0], [-1.0, 1.0]]
    assert ref.basis(5, 2)[1].tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]


def test_reference_by_hand_and_against_lstsq():
    rng = np.random.default_rng(0)
    D, T, K = 3, 300, 4
    bounds = np.array([-5, 10, 10, 140, 280, 400])  # clamped at both ends, one empty segment
    assert ref.segments(bounds, T) == [(0, 10), (10, 10), (10, 140), (140, 280), (280, 300)]
    x = rng.standard_normal((D, T)).astype(np.float32)
    flags = (rng.random((D, T)) < 0.1).astype(np.uint8)
    model = rng.standard_normal((D, T)).astype(np.float32)
    N, r, hits, aN, ar = ref.normal_equations(x, bounds, K, flags=flags, model=model)
    assert N.shape == (D, 5, K, K) and not N[:, 1].any() and not hits[:, 1].any()
    d, s, (lo, hi) = 1, 2, (10, 140)
    keep = flags[d, lo:hi] == 0
    P = ref.basis(hi - lo, K)[:, keep]
    y = (x[d, lo:hi].astype(np.float64) - model[d, lo:hi])[keep]
    np.testing.assert_allclose(N[d, s], P @ P.T, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r[d, s], P @ y, rtol=1e-12, atol=1e-13)
    assert hits[d, s] == keep.sum() and N[d, s, 0, 0] == keep.sum() and np.all(aN >= np.abs(N)) and np.all(ar >= np.abs(r))
    a, ok = ref.fit(x, bounds, K, flags=flags, model=model, min_hits=11)
    assert ok.tolist() == [[False, False, True, True, True]] * D  # the segment of 10 samples; the empty one
    np.testing.assert_allclose(a[d, s], np.linalg.lstsq(P.T, y, rcond=None)[0], rtol=1e-10)
    # apply: outside the segments nothing moves; a polynomial put in comes out
    coeffs = rng.uniform(-1, 1, (D, 5, K))
    zero = np.zeros((D, T), np.float32)
    drift = ref.apply(zero, bounds[2:5], coeffs[:, 2:4], sign=+1)
    assert not drift[:, :10].any() and not drift[:, 280:].any() and drift[:, 10:280].all()
    assert np.array_equal(ref.apply(drift, bounds[2:5], coeffs[:, 2:4], sign=-1), zero)
    a2, ok2 = ref.fit(drift, bounds[2:5], K)
    assert ok2.all() and np.abs(a2 - coeffs[:, 2:4]).max() <= 1e-6
    y2, f2, _, _ = ref.filter_subscans(drift, drift, bounds[2:5], np.zeros(T, np.uint8), K - 1)
    assert np.abs(y2).max() <= 8 * 2.0**-24 * np.abs(drift).max() and not f2.any()


def test_python_refusals_come_before_any_device_call():
    """Host tensors: every refusal of the C entries, and bounds that do not ascend, raise ValueError in Python, and a
    valid call raises at the last check, "x must be a device tensor", without touching a device."""
    import torch

    D, T, S, K = 4, 32, 3, 3
    x = torch.zeros((D, T), dtype=torch.float32)
    a = torch.zeros((D, S, K), dtype=torch.float64)
    flags = torch.zeros((D, T), dtype=torch.uint8)
    bounds = np.array([0, 10, 20, 32], np.int32)
    last = "x must be a device tensor"
    for good in (lambda: subscans.normal_equations(x, bounds, K, flags=flags, model=x), lambda: subscans.fit(x, bounds, K, flags=flags, model=x),
                 lambda: subscans.apply(x, bounds, a), lambda: subscans.inject_drifts(x, torch.as_tensor(bounds), a),
                 lambda: subscans.normal_equations(x, [-3, 5, 5, 40], 8), lambda: subscans.apply(x, bounds.astype(np.int64), a, out=x, sign=1)):
        with pytest.raises(ValueError, match=last):
            good()
    ne, ap = subscans.normal_equations, subscans.apply
    bad = [
        lambda: ne(x.double(), bounds, K), lambda: ne(x[:0], bounds, K), lambda: ne(x[:, ::2], bounds[:2], K), lambda: ne(x, bounds, 0),
        lambda: ne(x, bounds, 9), lambda: ne(x, bounds, 2.5), lambda: ne(x, bounds[:1], K), lambda: ne(x, bounds[None], K),
        lambda: ne(x, bounds.astype(np.float64), K), lambda: ne(x, bounds[::-1].copy(), K), lambda: ne(x, [0, 20, 10, 32], K),
        lambda: ne(x, torch.as_tensor(bounds).double(), K), lambda: ne(x, np.array([0, 2**31]), K), lambda: ne(x, bounds, K, flags=flags[:, :5]),
        lambda: ne(x, bounds, K, flags=flags.float()), lambda: ne(x, bounds, K, model=x[:2]), lambda: ne(x, bounds, K, model=x.double()),
        lambda: subscans.fit(x, bounds, K, min_hits=-1), lambda: subscans.fit(x, bounds, K, min_hits=2.5), lambda: subscans.fit(x, bounds, K, rcond=1.0),
        lambda: subscans.fit(x, bounds, K, rcond=-1e-3), lambda: ap(x, bounds, a, sign=0), lambda: ap(x, bounds, a, sign=2), lambda: ap(x, bounds, a[:, :2]),
        lambda: ap(x, bounds, a[:3]), lambda: ap(x, bounds, a.float()), lambda: ap(x, bounds, a[:, :, 0]), lambda: ap(x, bounds, torch.zeros((D, S, 9), dtype=torch.float64)),
        lambda: ap(x, bounds[:3], a), lambda: ap(x, bounds, a, out=torch.zeros((D, T + 1))), lambda: ap(x, bounds, a, out=torch.zeros((D, T), dtype=torch.float64)),
        lambda: subscans.inject_drifts(x, bounds, a[:, :2]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError) as err:
            call()
        assert last not in str(err.value), f"refusal {i} got as far as the device check"
    buf = torch.zeros(D * T + 8, dtype=torch.float32)  # an output that overlaps x without being x
    xv, yv = torch.as_strided(buf, (D, T), (T, 1), 0), torch.as_strided(buf, (D, T), (T, 1), 4)
    with pytest.raises(ValueError, match="overlap"):
        ap(xv, bounds, a, out=yv)


def test_tod_method_refusals():
    from maria_amd.sim import TOD, Coordinates

    T = 16
    coords = Coordinates(np.arange(T) / 10.0, np.linspace(0, 1, T), np.full(T, 1.0))
    tod = TOD({"a": np.zeros((3, T), np.float32)}, dets=None, coords=coords)
    for bad in (lambda: tod.filter_subscans(order=8), lambda: tod.filter_subscans(order=-1), lambda: tod.filter_subscans(order=1.5),
                lambda: tod.filter_subscans(min_hits=-1), lambda: tod.filter_subscans(rcond=1.0), lambda: tod.filter_subscans(turn_frac=2.0),
                lambda: tod.filter_subscans(bounds=[0, 9, 4, 16]), lambda: tod.filter_subscans(bounds=[0]), lambda: tod.filter_subscans(bounds=[0.0, 16.0]),
                lambda: tod.filter_subscans(into="b")):
        with pytest.raises(ValueError):
            bad()
