"""tests/pointing_ref.py on the CPU: the exact offsets, the float32 restatement, eps and the sharpness of the
four cases from the reference alone, the accepted sets against a brute-force search, and the acceptance check against
pixels moved on purpose."""

import numpy as np
import pointing_ref as pr
import pytest

CASES = pr.cases()
IDS = [c.name for c in CASES]


def _nearest(case):
    """The reference's own nearest pixel of every sample, (rows, cols)."""
    rows, _ = pr.accepted(case.exact[..., 1], case.eta.first, case.eta.step, case.eta.n, 0.0)
    cols, _ = pr.accepted(case.exact[..., 0], case.xi.first, case.xi.step, case.xi.n, 0.0)
    return rows, cols


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_offsets_in_float64_and_longdouble_agree(case):
    x64 = pr.exact_offsets(*case.pointing, dtype=np.float64)
    assert case.exact.dtype == np.float64 and case.exact.shape == (37, 3001, 2)
    assert np.abs(x64 - case.exact).max() <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_offsets_are_what_sample_maps_uses(case, monkeypatch):
    """sample_maps hands its own offsets to sample_channel: the very float32 numbers of oracle_offsets."""
    from oracle import hotpath, mapsample

    t, az, el, off, transform, centre = case.inputs
    seen = []

    def spy(offsets, eta, xi, channel_map, stokes_weights, bilinear=True):
        seen.append(np.array(offsets))
        return np.zeros(offsets.shape[:-1])

    monkeypatch.setattr(mapsample, "sample_channel", spy)
    az_d, el_d = hotpath.broadcast(off, az, el)
    mapsample.sample_maps(az_d, el_d, t, None, None, np.array([1.0, -1.0]), np.array([-1.0, 1.0]), centre, np.zeros((1, 1, 2, 2), np.float32),
                          np.ones((len(off), 1)), cal_scalars=[1.0], transform_stack=transform)
    assert len(seen) == 1 and seen[0].dtype == np.float32
    np.testing.assert_array_equal(seen[0].astype(np.float64), pr.oracle_offsets(*case.pointing))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_sharp_and_is_what_it_says(case):
    """eps <= 1.2e-6 rad and at most a quarter of the samples with two pixels to choose from -- from the reference alone;
    samples beyond every end of both axes; zero on no node and on no midpoint; every plane below 2^24 pixels (an index is
    exact in a float32 TOD); W's offsets pass 0.1 rad inside one wave."""
    assert case.eps == pr.epsilon(*case.pointing) == pr.epsilon(*case.pointing, exact=case.exact)
    share = pr.ambiguous_share(*case.sets)
    print(f"case {case.name}: E_oracle {case.e_oracle:.3e} eps {case.eps:.3e} ambiguous {share:.4f} grid {case.eta.n} x {case.xi.n} "
          f"off-map {case.off_map_shares()}")
    assert pr.DEVICE_BOUND < case.eps <= pr.EPS_MAX
    assert share <= pr.AMBIGUOUS_MAX
    assert all(s > 0 for s in case.off_map_shares())
    for ax in (case.eta, case.xi):
        assert min(abs(ax.c_frac - v) for v in (0.0, 0.5, 1.0)) > 0.1
        assert ax.n >= 2 and abs(ax.step) == case.pixel
    assert case.eta.step < 0 < case.xi.step
    assert case.eta.n * case.xi.n < 2**24
    far = np.hypot(case.exact[..., 0], case.exact[..., 1]).max()
    if case.name == "W":
        hit = case.mixed_wave()
        assert hit is not None and far > 0.11
        d, s = hit
        r2 = np.sin(np.hypot(*np.moveaxis(case.exact[d, s : s + pr.WAVE], -1, 0))) ** 2
        assert s % pr.WAVE == 0 and len(r2) == pr.WAVE and r2.min() < pr.R2_FAR < r2.max()
    else:
        assert far < 0.03 and case.mixed_wave() is None
    if case.name in "BC":
        assert min(case.eta.n, case.xi.n) > 700  # pixel indices in the hundreds and beyond


def _brute(x, first, step, n, eps):
    nodes = first + step * np.arange(n)
    idx = np.stack([np.abs(nodes[None, :] - p[:, None]).argmin(axis=1) for p in (x - eps, x, x + eps)])
    return idx.min(axis=0), idx.max(axis=0)


@pytest.mark.parametrize("step", [0.25, -0.25, 3e-5, -2e-5])
def test_accepted_matches_a_brute_force_search(step):
    rng = np.random.default_rng(5)
    n, first = 41, -0.37 * step - 20 * step
    last = first + (n - 1) * step
    eps = 0.02 * abs(step)
    # inside the axis, within eps of either end, and beyond both ends
    x = np.concatenate([rng.uniform(min(first, last) - 3 * abs(step), max(first, last) + 3 * abs(step), 20000),
                        first + rng.uniform(-2, 2, 500) * eps, last + rng.uniform(-2, 2, 500) * eps,
                        first + step * (rng.integers(0, n - 1, 2000) + 0.5) + rng.uniform(-2, 2, 2000) * eps])
    lo, hi = pr.accepted(x, first, step, n, eps)
    blo, bhi = _brute(x, first, step, n, eps)
    np.testing.assert_array_equal(lo, blo)
    np.testing.assert_array_equal(hi, bhi)
    assert lo.min() == 0 and hi.max() == n - 1 and (hi - lo).max() == 1 and 0.02 < (hi > lo).mean() < 0.2
    assert ((x < min(first, last) - eps) & (lo == hi)).any() and ((x > max(first, last) + eps) & (lo == hi)).any()


@pytest.mark.parametrize("step", [0.25, -0.25])
def test_accepted_on_a_midpoint_and_at_the_ends(step):
    """Exactly between nodes 2 and 3 (binary fractions: no rounding): both with any eps > 0, one of the two with none; the
    end nodes for points beyond the ends, however far."""
    first, n = 1.0, 8
    mid = first + 2.5 * step
    lo, hi = pr.accepted(np.array([mid]), first, step, n, 1e-9)
    assert (lo[0], hi[0]) == (2, 3)
    lo, hi = pr.accepted(np.array([mid]), first, step, n, 0.0)
    assert lo[0] == hi[0] and lo[0] in (2, 3)
    last = first + (n - 1) * step
    lo, hi = pr.accepted(np.array([first - 40 * step, first - 0.5 * step, last + 0.5 * step, last + 40 * step]), first, step, n, 1e-9)
    np.testing.assert_array_equal(lo, [0, 0, n - 1, n - 1])
    np.testing.assert_array_equal(hi, [0, 0, n - 1, n - 1])
    # within eps of the last midpoint: the end node and its neighbour
    lo, hi = pr.accepted(np.array([last - 0.5 * step]), first, step, n, 1e-9)
    assert (lo[0], hi[0]) == (n - 2, n - 1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_acceptance_check_rejects_and_passes_what_it_should(case):
    lo_e, hi_e, lo_x, hi_x = sets = case.sets
    rows, cols = _nearest(case)
    assert pr.check_pixels(rows, cols, *sets).all()
    for axis, (lo, hi, n) in enumerate(((lo_e, hi_e, case.eta.n), (lo_x, hi_x, case.xi.n))):
        def moved(where, to):
            r, c = rows.copy(), cols.copy()
            (r if axis == 0 else c)[where] = to
            ok = pr.check_pixels(r, c, *sets)
            return bool(ok[where]), int((~ok).sum())

        # an unambiguous sample inside the axis, one pixel either way: rejected, and it alone
        single = np.argwhere((lo == hi) & (lo > 0) & (lo < n - 1))
        assert len(single) > 0
        w = tuple(single[len(single) // 2])
        for step in (-1, 1):
            assert moved(w, lo[w] + step) == (False, 1)
        # a sample at an end node: one pixel into the map is rejected
        for edge, step in ((0, 1), (n - 1, -1)):
            at = np.argwhere((lo == hi) & (lo == edge))
            assert len(at) > 0 and moved(tuple(at[0]), edge + step) == (False, 1)
        # an ambiguous sample: either accepted pixel passes, the pixels beyond both do not
        pair = np.argwhere((hi == lo + 1) & (lo > 0) & (hi < n - 1))
        assert len(pair) > 0
        w = tuple(pair[len(pair) // 2])
        assert moved(w, lo[w]) == (True, 0) and moved(w, hi[w]) == (True, 0)
        assert moved(w, lo[w] - 1) == (False, 1) and moved(w, hi[w] + 1) == (False, 1)
