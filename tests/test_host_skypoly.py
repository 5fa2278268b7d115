"""maria_amd.sky_polynomial without a device: the basis against numpy, the reference of tests/skypoly_ref.py
against numpy.linalg.lstsq sample by sample, every refusal of the Python layer, and the margins of the fixtures the
device tests use: their smallest pivots, and the size of the mistakes the device tests' bounds would see."""

import numpy as np
import pytest
import skypoly_ref as ref


def test_n_terms_and_basis_against_numpy():
    from maria_amd import sky_polynomial as sp

    assert [sp.n_terms(o) for o in (0, 1, 2)] == [1, 3, 6] and sp.MAX_TERMS == 6
    rng = np.random.default_rng(0)
    off = rng.uniform(-0.5, 0.5, (40, 2)) + [3.0, -2.0]
    groups = rng.integers(-1, 3, 40).astype(np.int32)
    groups[:3] = [0, 1, 2]
    for order in (0, 1, 2):
        P = sp.basis(off, order, groups=groups, n_groups=3)
        assert P.dtype == np.float64 and P.shape == (40, sp.n_terms(order)) and P.flags.c_contiguous
        np.testing.assert_allclose(P, ref.basis(off, order, groups, 3), rtol=0, atol=4e-16)
        assert not P[groups < 0].any() and np.all(P[groups >= 0, 0] == 1.0) and np.abs(P).max() <= 1.0
    P = sp.basis(off, 2, groups=groups, n_groups=3)
    for g in range(3):
        rows = groups == g
        xy = off[rows] - off[rows].mean(axis=0)
        xy = xy / np.hypot(xy[:, 0], xy[:, 1]).max()
        want = np.stack([np.ones(rows.sum()), xy[:, 0], xy[:, 1], xy[:, 0] ** 2, xy[:, 0] * xy[:, 1], xy[:, 1] ** 2], axis=1)
        np.testing.assert_allclose(P[rows], want, rtol=0, atol=4e-16)
        assert abs(np.hypot(P[rows, 1], P[rows, 2]).max() - 1.0) < 1e-15 and np.abs(P[rows, 1:3].mean(axis=0)).max() < 1e-15
    # one group, one detector (radius 0 -> 1), and groups=None
    np.testing.assert_array_equal(sp.basis([[2.0, 3.0]], 2), [[1, 0, 0, 0, 0, 0]])
    np.testing.assert_allclose(sp.basis(off, 1), ref.basis(off, 1), rtol=0, atol=4e-16)


@pytest.mark.parametrize("K", range(1, 7))
def test_the_reference_against_lstsq(K):
    """Per sample: c minimises sum_d (v_d / 1) (P c - (x - off) u / v)^2 where u = w g, v = w g^2: the weighted least squares
    numpy.linalg.lstsq solves on rows scaled by sqrt(v)."""
    case = ref.case(63, 40, 3, K, 7 + K, exact=False)
    x, P, groups, flags = case["x"], case["P"], case["groups"], case["flags"]
    gain = np.where(case["v"] > 0, np.random.default_rng(K).uniform(0.7, 1.3, 63), 0.0)
    u, v = gain, gain * gain  # unit weights: the gain-weighted fit of fit_sky
    c, ok, hits, N, r, piv = ref.fit(x, P, u, v, off=case["off"], groups=groups, n_groups=3, flags=flags, model=case["model"], min_hits=K)
    term = x.astype(np.float64) - case["model"].astype(np.float64) - case["off"][:, None]
    checked = 0
    for g in range(3):
        for t in range(40):
            rows = np.flatnonzero((groups == g) & (v > 0) & (flags[:, t] == 0))
            assert hits[g, t] == rows.size
            if not ok[g, t]:
                assert rows.size < K or piv[g, :, t].min() < 1e-10 or not np.all(np.isfinite(piv[g, :, t]))
                assert not c[g, :, t].any()
                continue
            want = np.linalg.lstsq(gain[rows, None] * P[rows], term[rows, t], rcond=None)[0]
            cond = np.linalg.cond(gain[rows, None] * P[rows]) ** 2
            assert np.abs(c[g, :, t] - want).max() <= 1e3 * 2.0**-53 * cond * np.abs(want).max(), (g, t)
            checked += 1
    assert checked >= 40 and not ok[case["special"][0], case["special"][1]] and not ok[case["special"][0], case["special"][3]]
    assert hits[case["special"][0], case["special"][2]] == K and hits[case["special"][0], case["special"][3]] == K - 1


def test_reference_application_and_removal():
    """apply is x + sign (e + h P c) rounded once; remove takes an injected surface out to the noise."""
    rng = np.random.default_rng(2)
    D, T, K = 9, 17, 3
    x = rng.standard_normal((D, T)).astype(np.float32)
    P, c = rng.uniform(-1, 1, (D, K)), rng.standard_normal((1, K, T))
    h, e = rng.uniform(0.5, 2, D), rng.standard_normal(D)
    groups = np.array([0, -1, 0, 0, 0, 0, 0, 0, 0])
    up = ref.apply(x, P, c, h, e=e, groups=groups, sign=+1)
    want = x + (e[:, None] + h[:, None] * np.einsum("dk,kt->dt", P, c[0])).astype(np.float32)
    assert np.array_equal(up[1], x[1]) and np.abs(up - want)[groups == 0].max() <= 2.0**-22 * np.abs(want).max()
    back = ref.apply(up, P, c, h, e=e, groups=groups, sign=-1)
    assert np.abs(back - x).max() <= 2.0**-22 * np.abs(up).max()


def test_python_refusals():
    import torch

    from maria_amd import sky_polynomial as sp

    D, T, K, G = 6, 50, 3, 2
    x = torch.zeros((D, T), dtype=torch.float32)
    P = torch.ones((D, K), dtype=torch.float64)
    u = torch.ones(D, dtype=torch.float64)
    c = torch.zeros((G, K, T), dtype=torch.float64)
    flags = torch.zeros((D, T), dtype=torch.uint8)
    groups = np.zeros(D, np.int32)
    bad = [
        lambda: sp.n_terms(3), lambda: sp.n_terms(-1), lambda: sp.n_terms(1.5), lambda: sp.n_terms(True),
        lambda: sp.basis(np.zeros((4, 3)), 1), lambda: sp.basis(np.zeros(4), 1), lambda: sp.basis(np.full((4, 2), np.nan), 1),
        lambda: sp.basis(np.zeros((4, 2)), 3), lambda: sp.basis(np.zeros((4, 2)), 1, groups=np.zeros(3, int)),
        lambda: sp.basis(np.zeros((4, 2)), 1, groups=np.zeros(4)), lambda: sp.basis(np.zeros((4, 2)), 1, n_groups=17),
        # fit
        lambda: sp.fit(x.double(), P, u, u), lambda: sp.fit(x[:0], P[:0], u[:0], u[:0]), lambda: sp.fit(x[:, ::2], P, u, u),
        lambda: sp.fit(x, P, u, u, n_groups=0), lambda: sp.fit(x, P, u, u, n_groups=17), lambda: sp.fit(x, P.float(), u, u),
        lambda: sp.fit(x, P[:3], u, u), lambda: sp.fit(x, torch.ones((D, 7), dtype=torch.float64), u, u),
        lambda: sp.fit(x, torch.ones((D, 0), dtype=torch.float64), u, u), lambda: sp.fit(x, P[:, 0], u, u),
        lambda: sp.fit(x, P, u.float(), u), lambda: sp.fit(x, P, u, u[:3]), lambda: sp.fit(x, P, u, u, off=u[:3]),
        lambda: sp.fit(x, P, u, u, groups=groups[:3]), lambda: sp.fit(x, P, u, u, groups=groups.astype(np.float64)),
        lambda: sp.fit(x, P, u, u, flags=flags[:, :5]), lambda: sp.fit(x, P, u, u, flags=flags.float()), lambda: sp.fit(x, P, u, u, model=x[:2]),
        lambda: sp.fit(x, P, u, u, min_hits=0), lambda: sp.fit(x, P, u, u, min_hits=2.5), lambda: sp.fit(x, P, u, u, min_hits=-1),
        lambda: sp.fit(x, P, u, u, rcond=1.0), lambda: sp.fit(x, P, u, u, rcond=-1e-3),
        lambda: sp.fit(x, P, u, u),  # a host tensor: the last refusal
        # apply
        lambda: sp.apply(x.double(), P, c, u), lambda: sp.apply(x, P.float(), c, u), lambda: sp.apply(x, P, c[0], u),
        lambda: sp.apply(x, P, c[:, :2], u), lambda: sp.apply(x, P, c[:, :, :5], u), lambda: sp.apply(x, P, c.float(), u),
        lambda: sp.apply(x, P, torch.zeros((17, K, T), dtype=torch.float64), u), lambda: sp.apply(x, P, c, u[:3]),
        lambda: sp.apply(x, P, c, u, e=u.float()), lambda: sp.apply(x, P, c, u, groups=groups[:2]), lambda: sp.apply(x, P, c, u, sign=0),
        lambda: sp.apply(x, P, c, u, sign=2), lambda: sp.apply(x, P, c, u, out=x[:, :5]), lambda: sp.apply(x, P, c, u, out=x.double()),
        lambda: sp.apply(x, P, c, u, out=torch.as_strided(x, (D, T - 1), (T, 1), 1)), lambda: sp.apply(x, P, c, u),
        # fit_sky
        lambda: sp.fit_sky(x, P[:, 0]), lambda: sp.fit_sky(x, P, min_dets=0), lambda: sp.fit_sky(x, P, min_dets=2.5),
        lambda: sp.fit_sky(x, P, min_dets=True), lambda: sp.fit_sky(x, P, n_iter=0), lambda: sp.fit_sky(x, P),
        lambda: sp.inject_gradient(x, P, c),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {i} did not raise")


def test_tod_method_refusals():
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    D, T = 12, 40
    rng = np.random.default_rng(0)
    dets = Detectors(rng.uniform(-1, 1, (D, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int))
    tod = TOD({"signal": np.zeros((D, T), np.float32)}, dets, Coordinates(np.arange(T) / 50.0, np.zeros(T), np.full(T, 1.0)), units="K_RJ")
    bad = [dict(order=3), dict(order=-1), dict(order=0.5), dict(groups="array"), dict(groups=np.full(D, -2)), dict(groups=np.arange(D) * 2),
           dict(groups=np.zeros(D - 1, int)), dict(min_hits=-1), dict(min_dets=0), dict(min_dets=1.5), dict(into="other"),
           dict(model=np.zeros((D, T + 1), np.float32)), dict(rcond=1.0), dict(n_iter=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            tod.remove_sky_polynomial(device="cpu", **kw)
            pytest.fail(f"{kw} did not raise")


def test_the_solve_fixtures_keep_away_from_rcond():
    """The inputs of the device's solve test: every pivot of every sample that has at least K rows is >= 1e-3, the
    sample with exactly K rows included; the rank-deficient variant (a duplicated column) has a pivot below 1e-12 in
    magnitude or not finite: neither verdict depends on a rounding of the reference or of the device."""
    smallest = {}
    for D, T, G in ref.SOLVE_CASES:
        for K in range(1, 7):
            case = ref.case(D, T, G, K, 100 * K + D, exact=False)
            c, ok, hits, N, r, piv = ref.fit(case["x"], case["P"], case["u"] * 0 + 1.0, case["v"], off=case["off"], groups=case["groups"],
                                             n_groups=G, flags=case["flags"], min_hits=1)
            enough = hits >= K
            assert case["special"] is not None and hits[case["special"][0], case["special"][2]] == K
            assert np.array_equal(ok, enough)
            low = float(piv.transpose(0, 2, 1)[enough].min())
            smallest[K] = min(smallest.get(K, 1.0), low)
            assert low >= 1e-3, (D, T, G, K, low)
            if K >= 2:
                P2 = case["P"].copy()
                P2[:, K - 1] = P2[:, 0 if K == 2 else 1]
                _, ok2, _, _, _, piv2 = ref.fit(case["x"], P2, case["v"], case["v"], groups=case["groups"], n_groups=G, flags=case["flags"], min_hits=1)
                last = piv2[:, K - 1, :][enough]
                assert not ok2.any() and np.all(~np.isfinite(last) | (np.abs(last) < 1e-12))
    print("smallest pivot per K:", {k: f"{v:.3g}" for k, v in smallest.items()})


def test_the_science_fixture_in_numpy():
    """61 detectors on a hexagonal lattice, T = 2000: the smallest pivot over all samples (0.97 at K = 3 and 0.38 at K = 6
    within a few per cent: the flags are random), and with the injected gains and offsets the residual rms over the
    unflagged samples within 0.5 % of sigma sqrt(1 - K / (0.95 D)) for the matching order and above 4 sigma for the order
    below.  (With gains fitted by fit_common_mode the residual is larger: DESIGN 3.36.)"""
    assert ref.hexagon().shape == (61, 2) and len({(round(a, 9), round(b, 9)) for a, b in ref.hexagon()}) == 61
    for K, lower in ((3, 0), (6, 1)):
        x, flags, pos, gains, offs, c, _ = ref.science(K)
        D = len(pos)
        assert abs(np.abs(c).max() - 20.0) < 1e-12 and 0.04 < flags.mean() < 0.06
        for order, matching in ((lower, False), ({3: 1, 6: 2}[K], True)):
            P = ref.basis(pos, order)
            k = P.shape[1]
            cc, ok, _, _, _, piv = ref.fit(x, P, gains, gains * gains, off=offs, flags=flags, min_hits=2 * k)
            rms = ref.residual_rms(ref.apply(x, P, cc, gains, e=offs), flags)
            print(f"injected K {K}, fitted K {k}: residual {rms:.4f} sigma, smallest pivot {piv.min():.3f}")
            assert ok.all()
            if matching:
                assert abs(rms / np.sqrt(1 - k / (0.95 * D)) - 1) <= 0.005
                assert abs(piv.min() / {3: 0.97, 6: 0.38}[K] - 1) <= 0.05
            else:
                assert rms > 4.0


def test_the_size_of_the_mistakes_the_bounds_see():
    """A sum that leaves out one row, adds a flagged one or is added in float32 misses the device test's bound
    (n + 1) 2^-53 sum|terms| by orders of magnitude; a coefficient that is wrong by 1e-10 of its size shows as a ratio
    above Higham's 4 K (3 K + 1) wherever the scaled matrix' condition number is below 1e3."""
    case = ref.case(65, 64, 1, 6, 3, exact=False)
    x, P, u, v, flags = case["x"], case["P"], case["u"], case["v"], case["flags"]
    N, r, hits, aN, ar = ref.sums(x, P, u, v, flags=flags, groups=case["groups"])
    bound = (hits[:, None, :] + 1) * 2.0**-53 * ar
    row = int(np.flatnonzero((case["groups"] == 0) & (v > 0))[3])
    f2 = flags.copy()
    f2[row] = 1
    miss = ref.sums(x, P, u, v, flags=f2, groups=case["groups"])[1]
    changed = flags[row] == 0
    live = bound[0, 1] > 0  # not the samples flagged in the whole group
    assert np.median((np.abs(miss - r)[0, 0] / np.where(live, bound[0, 0], 1.0))[changed & live]) > 1e12
    single = ref.sums(x, P.astype(np.float32).astype(np.float64), u, v, flags=flags, groups=case["groups"])[1]
    assert np.median((np.abs(single - r)[0, 1] / np.where(live, bound[0, 1], 1.0))[live]) > 1e5
    M, _ = ref.scaled(N[0], 6)
    kappa = np.linalg.cond(M[hits[0] >= 12])
    assert np.median(kappa) < 1e3
    assert 1e-10 / (2.0**-53 * np.median(kappa)) > 4 * 6 * 19
