"""tests/krj_ref.py on the CPU: the exact lookup against the float32 oracle, the float32 chain's distance from
the exact elevation per case, the sharpness of the zigzag tables under the allowance -- a neighbouring cell and a dropped
kink must show --, the shares of exempt and straddling samples, and that every case contains the form it names."""

import krj_ref as kr
import numpy as np
import pytest

CASES = kr.cases()
case_param = pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
# the cases whose detectors come within 6 degrees of the zenith: asin(im) is ill-conditioned there (an ulp of im, 6e-8, is
# 6e-8 / cos(el) of elevation: 1e-5 rad at 89.7 deg, sqrt(2 x 6e-8) = 3.5e-4 rad at the zenith itself) in every float32 chain
NEAR_ZENITH = {"zenith": 2e-5, "off_zenith": 4e-4}


def test_den_exact_against_the_float32_oracle():
    """den_exact on the collapsed _cal_tables against oracle.hotpath.calibrate_to_krj (float32: the weight, two products
    and a sum, the quotient, the 1e-12 and k_B factors: eight roundings of 2^-24, a sample's distance to its node in ulps of
    el on the weight), NaNs alike; elevations on nodes, within an ulp of them, off both ends."""
    from test_gpu_calibration import _cal_tables

    from maria_amd import pipeline_host
    from oracle import hotpath

    tables, polarized = _cal_tables(2), [True, False]
    axis, dens = pipeline_host.collapse_calibration(tables, 280.0, 2.5, polarized)
    ax32 = axis.astype(np.float32)
    rng = np.random.default_rng(2)
    el = np.concatenate([rng.uniform(ax32[0] - 0.01, ax32[-1] + 0.01, 4000).astype(np.float32), ax32, np.nextafter(ax32, np.float32(0)),
                         np.nextafter(ax32, np.float32(2))])
    el_det = np.stack([el, el[::-1]])
    ref32 = hotpath.calibrate_to_krj(np.ones(el_det.shape, np.float32), [0, 1], tables, 280.0, 2.5, el_det, polarized).astype(np.float64)
    worst = 0.0
    for b in range(2):
        den = kr.den_exact(ax32, dens[b], el_det[b].astype(np.float64))
        assert np.array_equal(np.isnan(den), np.isnan(ref32[b])) and 0 < np.isnan(den).sum() < den.size / 2
        ok = np.isfinite(den)
        worst = max(worst, float(np.abs(1.0 / den[ok] / ref32[b][ok] - 1).max()))
    print(f"den_exact against the float32 oracle: {worst:.2e}")
    assert worst <= 8 * kr.ULP


@case_param
def test_float32_chain_stays_near_the_exact_elevation(case):
    """delta_chain below 1e-6 rad, so that B_el is dominated by the project's grant -- away from the zenith; the two
    tracks that end there state what the conditioning of asin costs instead."""
    print(f"case {case.name}: delta_chain {case.delta_chain:.3e} rad, largest chord deviation below the gate {case.chord.max():.3e}")
    assert 0 < case.delta_chain < NEAR_ZENITH.get(case.name, 1e-6)
    assert case.b_el.shape == (1, case.shape[1]) and (case.b_el >= kr.GRANT + case.delta_chain).all()
    far = np.cos(case.el).min()
    assert (far < 0.1) == (case.name in NEAR_ZENITH)


@pytest.mark.parametrize("kind", ["zigzag", "nonuniform"])
@case_param
def test_zigzag_is_sharp_under_the_allowance(case, kind):
    """A neighbouring cell in place of the sample's own, or one line through the lower cell for a row that passes a node
    (the kink dropped), exceeds tol on at least 30 % of the samples it touches."""
    axis, values = case.table(kind)
    den, tol = case.den(kind), case.tol(kind)
    ok = np.isfinite(den)
    shares = []
    for step in (-1, 1):
        hit = np.zeros(den.shape, bool)
        n = 0
        for r, b in enumerate(case.band):
            i = kr.cell_of(axis, case.el[r])
            j = i + step
            m = ok[r] & (j >= 0) & (j <= len(axis) - 2)
            wrong = kr.den_in_cell(axis, values[b], case.el[r], np.clip(j, 0, len(axis) - 2))
            hit[r] = m & (np.abs(wrong / den[r] - 1) > tol[r])
            n += int(m.sum())
        shares.append(hit.sum() / n if n else 1.0)  # (no such neighbour: the samples all sit in an end cell)
    # the kink dropped: per tile and row, every sample on the line of the row's lowest cell in the tile
    form = case.form_of_samples(kind)
    touched = missed = 0
    for r, b in enumerate(case.band):
        i = kr.cell_of(axis, case.el[r])
        for s0 in range(0, case.shape[1], kr.TILE):
            s = slice(s0, s0 + kr.TILE)
            if form[r, s0] != kr.KINK or not ok[r, s].all():
                continue
            low = i[s].min()
            above = i[s] > low
            wrong = kr.den_in_cell(axis, values[b], case.el[r, s], low)
            touched += int(above.sum())
            missed += int((above & (np.abs(wrong / den[r, s] - 1) > tol[r, s])).sum())
    print(f"case {case.name} {kind}: a neighbouring cell shows on {shares[0]:.3f} / {shares[1]:.3f} of the samples, a dropped kink on "
          f"{missed} of {touched}; largest tol {np.nanmax(tol):.2e}")
    assert min(shares) >= 0.3
    assert touched == 0 or missed >= 0.3 * touched
    if case.name in ("kink", "descending", "curved_under"):
        assert touched > 1000


@pytest.mark.parametrize("kind", kr.KINDS)
@case_param
def test_exempt_and_straddling_shares(case, kind):
    """At most 1e-3 of an off-axis case within B_el of an end of the axis (exempt from the NaN pattern); at most 5 % of the
    four-sample groups with a straddle allowance; the off-axis cases have NaNs and finite samples, the others no NaN."""
    exempt, nan = case.exempt(kind), np.isnan(case.den(kind))
    print(f"case {case.name} {kind}: exempt {exempt.mean():.2e}, straddling groups {case.straddle_share(kind):.4f}, NaN {nan.mean():.3f}")
    assert exempt.mean() <= 1e-3
    assert case.straddle_share(kind) <= 0.05
    if kind.startswith("ramp"):
        assert case.straddle_share(kind) == 0.0  # den = el has no kink
    if case.name in ("off_low", "off_high", "tiles"):
        assert 0.05 < nan.mean() < 0.5
    else:
        assert not nan.any()
    on = ~nan
    if kind.startswith("ramp"):
        assert np.abs(case.den(kind)[on] - case.el[on]).max() <= 1e-12


@case_param
def test_case_contains_the_form_it_names(case):
    D, T = case.shape
    assert case.el.shape == (D, T) and case.bore_el.dtype == np.float32 and case.off.dtype == np.float32
    if not case.name.startswith("ragged"):
        assert (D, T) == (37, 3 * 1024 + 5) and D % kr.TILE_DET == 5
    for kind, form in case.contains:
        for gate in (None, kr.CURVATURE_GATE):
            f = case.forms(kind, gate)
            assert f.shape == (-(-T // kr.TILE), D)
            assert (f == kr.FORMS.index(form)).any(), (case.name, kind, form, gate, np.bincount(f.ravel(), minlength=5))


def test_the_cases_sit_where_they_say():
    """sweep: either side of hi - lo <= 0.04; kink and the gate tracks: a node inside a thread's four samples; curved:
    every tile past the gate, the two gate tracks 15 % either side of 1e-6 rad; wide: the last ring past r^2 = 0.09;
    steep: both thresholds (0.3 and 0.25 in cos) crossed; ragged: rows that are no multiple of four floats."""
    for c in CASES:
        rng = [float(hi) - float(lo) for lo, hi, _, _ in kr.tile_ranges(c.bore_el)]
        if c.name.startswith("sweep"):
            full = rng[:3]
            assert all(0.0385 < r < 0.04 for r in full) if c.name.endswith("under") else all(0.04 < r < 0.0415 for r in full)
            radii = np.degrees(np.hypot(c.off[:, 0], c.off[:, 1]))
            assert {round(float(r), 2) for r in radii} == {0.0, 0.25, 1.0, 1.41}
        if c.name in ("kink", "curved_under"):
            assert c.straddle_share("zigzag") > 0
    dev = {n: kr.chord_deviation(kr.case(n).bore_el).max() for n in ("curved", "curved_under", "curved_over")}
    assert dev["curved"] > 1e-4 and 0.8e-6 < dev["curved_under"] < 0.93e-6 and 1.07e-6 < dev["curved_over"] < 1.25e-6
    assert kr.case("curved").curved_tiles.all() and not kr.case("curved_under").curved_tiles.any() and kr.case("curved_over").curved_tiles.any()
    assert kr.case("curved_under").chord.max() == dev["curved_under"] and kr.case("curved_over").chord.max() < 1e-6
    for n in ("wide_45", "wide_60"):
        r2 = (kr.case(n).off.astype(np.float64) ** 2).sum(axis=1)
        assert (r2 > 0.09).sum() >= 8 and ((r2 > 0) & (r2 < 0.09)).sum() >= 24
    c0 = np.cos(kr.case("steep").bore_el.astype(np.float64))
    assert c0.max() > 0.3 > 0.25 > c0.min()
    assert {c.pad for c in CASES if c.name.startswith("ragged")} == {3}
    assert {c.shape for c in CASES if c.name.startswith("ragged")} == {(D, T) for D in (1, 17) for T in (1, 3, 1023, 1025)}
    assert np.array_equal(kr.case("descending").bore_el, kr.case("lin").bore_el[::-1])


def test_tables():
    for kind in kr.KINDS:
        axis, values = kr.table(kind)
        assert axis.dtype == values.dtype == np.float32 and values.shape == (2, len(axis)) and (np.diff(axis) > 0).all()
    a3, v3 = kr.table("ramp3")
    a200, v200 = kr.table("ramp200")
    assert len(a3) == 3 and len(a200) == 200 and np.array_equal(v3[1], a3) and np.array_equal(v200[0], a200)
    assert 0.34 < np.degrees(np.diff(a200)).mean() < 0.36
    az, vz = kr.table("zigzag")
    assert len(az) == 33 and abs(np.degrees(az[0]) - 20) < 1e-5 and abs(np.degrees(az[-1]) - 90.1) < 1e-5
    step = np.diff(az.astype(np.float64))
    assert np.ptp(step[:-1]) < 1e-6 and step[-1] > step[0] + 1e-3  # the last node off the uniform step
    g = kr.slopes(az, vz[0])
    assert (np.sign(g[:-1]) == -np.sign(g[1:])).all() and 0.4 < np.abs(g).min() and np.abs(g).max() < 0.7
    assert np.allclose(vz[1] / vz[0], 1.25, rtol=1e-6)
    an, vn = kr.table("nonuniform")
    sn = np.diff(an.astype(np.float64))
    assert len(an) == 33 and 2.9 < sn.max() / sn.min() < 3.1 and np.array_equal(vn, vz) and an[0] == az[0] and abs(an[-1] - az[-1]) < 1e-6
