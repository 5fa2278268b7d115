"""tests/atm_los_ref.py on the CPU: the exact chain against pointing_ref's and against float64, both float32
restatements against it, the conditions on eps, case R's shares, case F's ratio, the triangle wave and the value bounds on
hand-made positions -- and, on a numpy model of the pixel kernel's arithmetic, that the unmutated model passes every check the
device is held to while each of the eight mutations of DESIGN 3.41 fails the check named for it, with its size against eps.

Every test prints the figures DESIGN 3.41 quotes ("atm los ref: ...")."""

import atm_los_ref as ar
import numpy as np
import pointing_ref as pr
import pytest

CASES = ar.CASE_NAMES


def _sci(a):
    return "[" + " ".join(f"{x:.2e}" for x in np.ravel(a)) + "]"


def test_exact_chain_against_pointing_ref_and_float64():
    """Step 1 as pointing_ref.exact_offsets states it: the offsets of every sample from a map centre, which that module
    obtains by its own steps 1 and 3, are -- taken as focal-plane offsets about that centre -- the same lines of sight.  And
    the longdouble evaluation against the same formulas in float64."""
    p = ar.case("S").problem
    dx, dy, az, el = ar.device_inputs(p)
    px, py, theta = ar._unit(dx, dy, az, el)
    centre = (float(np.float32(az.mean())), float(el.mean()))
    xi_eta = pr.exact_offsets(np.stack([dx, dy], axis=1), az, el, None, centre)  # [D, Ta, 2] float64
    D, Ta = theta.shape
    qx, qy, qt = ar._unit(xi_eta[..., 0].ravel(), xi_eta[..., 1].ravel(), np.array([centre[0]]), np.array([centre[1]]))
    for a, b in ((px, qx), (py, qy), (theta, qt)):
        assert float(np.abs(a - b.reshape(D, Ta)).max()) <= 1e-12  # the float64 store of offsets below 0.02 rad, times 1 / im^2
    fx, fy, ft = ar._unit(dx, dy, az, el, np.float64)
    worst = max(float(np.abs(a - b).max()) for a, b in ((px, fx), (py, fy), (theta, ft)))
    print(f"atm los ref: longdouble against float64: {worst:.2e}")
    assert worst <= 2e-15  # a dozen float64 roundings of numbers below 1


@pytest.mark.parametrize("name", CASES)
def test_both_restatements_against_the_exact_chain(name):
    """The oracle's chain and the kernel's own form are float32 evaluations of the exact projection: a few float32 roundings
    of numbers below 1 apart from it, and no closer than one."""
    c = ar.case(name)
    for which, (e_unit, e_theta) in c.errors.items():
        print(f"atm los ref: case {name}: {which}: E_unit = {e_unit:.2e}, E_theta = {e_theta:.2e}")
        assert 2.0 ** -25 < e_unit <= 16 * ar.U24 and 2.0 ** -25 < e_theta <= 16 * ar.U24


@pytest.mark.parametrize("name", CASES)
def test_eps_is_sharp_enough(name):
    c = ar.case(name)
    eps = c.eps()
    print(f"atm los ref: case {name}: E_unit = {c.e_unit:.2e}, h / res up to {c.h_over_res.max():.0f}, |delta| up to {c.exact.delta.max():.1f}, "
          f"eps = {_sci(eps)}; literal {_sci(c.eps('literal'))}")
    assert (eps <= ar.EPS_CAP).all()
    assert c.exact.pixel == ((True, False, False) if name == "N" else (True,) * len(eps))
    if name != "R":  # every sample well inside every grid: no NaN is expected, the rim rule is idle
        assert ar.rim_margin(c.exact.pos, c.shapes)[0].min() > 1.0
    if name == "W":
        assert c.exact.delta.max() > 40.0
    if name == "L":
        assert c.exact.pos[..., 0].min() >= 6000.0 and np.allclose(eps, ar.case("S").eps()[:3], rtol=1e-6)
    if name == "F":
        assert min(abs(l[a]).min() for l in c.problem["layers"] for a in ("extrusion", "cross_section")) >= 30e3
        assert (c.eps("literal") >= 2 * eps).all()
        assert np.allclose(eps, ar.case("S").eps()[:3], rtol=1e-6)  # the pixel route: the same eps as S


def test_case_r_puts_samples_off_every_side():
    c = ar.case("R")
    eps = c.eps()[:, None, None, None]
    _, sides = ar.rim_margin(c.exact.pos, c.shapes)  # [L, 4, D, Ta]
    beyond = (sides < -eps).mean(axis=(2, 3))
    near = (np.abs(sides) <= eps).any(axis=(0, 1)).mean()
    print(f"atm los ref: case R: share beyond each side by more than eps, per layer: {np.array2string(beyond, precision=4)}; within eps of a rim: {near:.2e}")
    assert (beyond.max(axis=0) >= 1e-3).all()
    assert near <= 1e-2
    must_nan, must_be_finite = ar.rim_classes(c.exact.pos, c.shapes, c.eps())
    assert must_nan.mean() > 0.05 and must_be_finite.mean() > 0.5 and not (must_nan & must_be_finite).any()


def test_triangle_wave_and_value_bounds_on_hand_made_positions():
    x = np.array([0.0, 0.25, 7.5, 8.0, 8.5, 15.75, 16.0, 23.0, 24.0, 100.0])
    assert np.array_equal(ar.tri(x), [0.0, 0.25, 7.5, 8.0, 7.5, 0.25, 0.0, 7.0, 8.0, 4.0])
    for axis in (0, 1):
        v = ar.axis_screen((40, 37), axis, "tri")
        assert v.dtype == np.float32 and v.min() == 0.0 and v.max() == 8.0
        pos = np.array([[3.25, 5.5], [7.75, 8.25], [38.999, 35.999], [16.5, 31.5]])
        assert np.allclose(ar.bilinear(v, pos), ar.tri(pos[:, axis]), rtol=0, atol=1e-13)  # linear between the nodes, kinks on nodes
        assert np.array_equal(ar.lipschitz(v, pos), np.ones(4))
        ramp = ar.axis_screen((40, 37), axis, "ramp")
        assert np.allclose(ar.bilinear(ramp, pos), pos[:, axis], rtol=0, atol=1e-13)
    # the blend on a hand-made screen, and L(x) from the cell of x and its neighbours only
    v = np.zeros((6, 6), np.float32)
    v[2, 3] = 4.0
    assert ar.bilinear(v, np.array([1.5, 2.5])) == 1.0 and ar.bilinear(v, np.array([2.0, 3.0])) == 4.0
    assert ar.lipschitz(v, np.array([0.5, 0.5])) == 0.0 and ar.lipschitz(v, np.array([0.5, 1.5])) == 4.0
    assert ar.lipschitz(v, np.array([4.5, 4.5])) == 0.0 and ar.lipschitz(v, np.array([3.5, 4.5])) == 4.0
    # a blend moved by d along either axis changes by at most d L(x): white noise, steps of a thousandth of a pixel
    rng = np.random.default_rng(1)
    w = rng.standard_normal((30, 30)).astype(np.float32)
    pos = rng.uniform(1.0, 28.0, (20000, 2))
    step = rng.uniform(-1e-3, 1e-3, pos.shape)
    moved = np.abs(ar.bilinear(w, pos + step) - ar.bilinear(w, pos))
    assert (moved <= np.abs(step).sum(axis=1) * ar.lipschitz(w, pos)).all()
    assert ar.layer_bound(w, pos, 0.0).max() == 3 * ar.U24 * float(np.abs(w).max())


def _model_band(c, pwv, mutation=None):
    return ar.band_model(c.problem, pwv, ar.unit_kernel(c.problem)[2], mutation)


@pytest.mark.parametrize("name", ["S", "W", "F", "R", "L"])
def test_the_unmutated_model_passes_every_check(name):
    """The pixel kernel's arithmetic in numpy, on the screens and through the checks the device gets: the bounds are not
    tighter than a correct float32 evaluation.  (Case N takes the general kernel: literal_model, below.)"""
    c = ar.case(name)
    for kt, pipe in ((1, False), (2, True)):
        j = ar.Judge(c)
        for l in (0, len(c.shapes) - 1):
            for axis in (0, 1):
                for kind in ("ramp", "tri") if name == "S" else ("tri",):
                    screens, amp = j.axis_run(l, axis, kind)
                    pwv, _ = ar.pixel_model(c.problem, screens, amp, kt=kt, pipe=pipe)
                    j.axis(l, axis, kind, pwv)
                    j.band(c.problem, pwv, _model_band(c, pwv))
        pwv, pos = ar.pixel_model(c.problem, c.noise, kt=kt, pipe=pipe)
        j.stack(pwv)
        ok = np.isfinite(pwv)
        assert (np.abs(pos - c.exact.pos)[:, ok].max(axis=(1, 2)) <= j.eps).all()
    print(f"atm los ref: case {name}: model: largest |model - exact| = {j.worst['position']:.2e} pixel, stack {j.worst['stack']:.3f}, band {j.worst['band']:.3f}")


@pytest.mark.parametrize("name", ["S", "F", "N"])
def test_the_literal_rule_stays_inside_its_own_eps(name):
    """The array search in float32 (MRX_OPT_AXIS_LITERAL; case N's layers 1 and 2 by default) against the exact positions:
    inside the literal eps -- and, on case F, outside the pixel route's: what the float64 anchor is for."""
    c = ar.case(name)
    err = np.abs(ar.literal_model(c.problem) - c.exact.pos).max(axis=(1, 2, 3))
    print(f"atm los ref: case {name}: literal rule: |model - exact| = {_sci(err)}")
    assert (err <= c.eps("literal")).all()
    if name == "F":
        assert (err > c.eps()).all()
    if name == "N":
        assert (err[1:] <= c.eps("general")[1:]).all()


# mutation -> (case, model arguments, the check that catches it): DESIGN 3.41's table
MUTATIONS = {
    1: ("L", {}, "tri"),                       # the anchor in float32: 6000 pixels from the first node it is spaced 4.9e-4 pixel
    2: ("S", {}, "stack"),                     # r0.y and r1.x swapped
    3: ("S", {}, "stack"),                     # we and wc swapped
    4: ("R", {}, "rim"),                       # half_e = n_e / 2: half a pixel beyond the far rim passes as inside
    5: ("S", {}, "tri"),                       # the anchors of the step before
    6: ("S", {"pipe": True}, "stack"),         # the ring's next slot
    7: ("S", {"kt": 2}, "tri"),                # the pair's second step on the first step's anchor
    8: ("W", {}, "band"),                      # guess_cell's weight with the first step's inverse, on a stretched axis
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_each_mutation_fails_its_check(mutation):
    name, kw, check = MUTATIONS[mutation]
    c = ar.case(name)
    j = ar.Judge(c)
    # (1: the bottom layer has the smallest eps; 6: the shifted ring never blends layer 0, blends layers 1 ... 6 one turn early --
    # which a single lit layer does not notice -- and layer 4 twice)
    top = 0 if mutation in (1, 6) else len(c.shapes) - 1
    if check == "band":
        pwv, _ = ar.pixel_model(c.problem, c.noise)
        j.band(c.problem, pwv, _model_band(c, pwv))
        with pytest.raises(AssertionError, match="band lookup"):
            j.band(c.problem, pwv, _model_band(c, pwv, mutation))
        print(f"atm los ref: mutation {mutation}: band lookup |loading - P| / bound = {j.worst['band']:.3g}")
        return
    if check == "stack":
        pwv, pos = ar.pixel_model(c.problem, c.noise, mutation=mutation, **kw)
        with pytest.raises(AssertionError, match="white-noise stack"):
            j.stack(pwv)
        print(f"atm los ref: mutation {mutation}: white-noise stack |pwv - ref| / bound = {j.worst['stack']:.3g}")
        # ... and the triangle waves see it too wherever the two weights differ or the wrong layer is lit
        screens, amp = j.axis_run(top, 0, "tri")
        with pytest.raises(AssertionError):
            j.axis(top, 0, "tri", ar.pixel_model(c.problem, screens, amp, mutation=mutation, **kw)[0])
        return
    screens, amp = j.axis_run(top, 0, "tri")
    pwv, pos = ar.pixel_model(c.problem, screens, amp, mutation=mutation, **kw)
    if check == "rim":
        with pytest.raises(AssertionError, match="beyond a rim came out finite"):
            j.axis(top, 0, "tri", pwv)
        wrong = float((np.isfinite(pwv) & j.must_nan).mean())
        print(f"atm los ref: mutation {mutation}: share of samples beyond a rim that came out finite = {wrong:.2e}")
        return
    with pytest.raises(AssertionError, match="tri"):
        j.axis(top, 0, "tri", pwv)
    print(f"atm los ref: mutation {mutation}: largest position error {np.abs(pos - c.exact.pos)[top].max():.2e} pixel against eps {j.eps[top]:.2e}")
