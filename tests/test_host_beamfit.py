"""The beam fit on the host (maria_amd/beamfit.py): the reference's Jacobian against central differences of
its own model, the reference fit on exact truth, every refusal before a device call, the beam's FWHM and angle from
known quadratic forms, and the two entries in the header and the binding table."""

import os
import re

import numpy as np
import pytest

import beamfit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("far", [0.0, 0.12], ids=["r=0.01", "r=0.12"])
def test_jacobian_against_central_differences(K, far):
    """Every column of the reference's Jacobian against (m(p + h) - m(p - h)) / 2h.  The columns of (dx, dy) hold the
    asin(r)/r factor constant: they differ from the differences by a relative r^2 / 3 to leading order, r the angle
    between the detector's direction and the frame's centre, and by no more than r^2; the others agree to the
    differences' own error.  ``far`` moves the frame's centre that many radians off the scan so that r^2 is 1.4e-2 and
    the neglected term shows."""
    case = R.make_case("ra/dec", drift=True, K=K, D=5)
    center = (case["center"][0] + far / np.cos(case["center"][1]), case["center"][1])
    G = R.rotations(case["az"], case["el"], case["transform"], center)
    src = case["src"].astype(np.float64)  # the track is relative to the centre
    p = R.start_of(case)[:4]
    p[:, 1:3] = case["truth"][:4, 1:3]
    ox, oy, oj = R.offsets(G, p[:, 1], p[:, 2], jac=True)
    r2 = float((ox * ox + oy * oy).max())
    u, v = ox - src[None, :, 0], oy - src[None, :, 1]
    # a source where the detectors point: the centre of the first detector's track
    shift = (float(np.median(ox[0])), float(np.median(oy[0])))
    u, v = u - shift[0], v - shift[1]
    J = R.jacobian(p, u, v, oj)

    def m_of(q):
        a, b = R.offsets(G, q[:, 1], q[:, 2])
        return R.model(q, a - src[None, :, 0] - shift[0], b - src[None, :, 1] - shift[1])[0]

    steps = R.scales(p) * 1e-5
    for k in range(K):
        hp, hm = p.copy(), p.copy()
        hp[:, k] += steps[:, k]
        hm[:, k] -= steps[:, k]
        num = (m_of(hp) - m_of(hm)) / (2.0 * steps[:, k, None])
        scale = np.abs(num).max(axis=1, keepdims=True)
        assert np.all(scale > 0)
        rel = float((np.abs(J[..., k] - num) / scale).max())
        print(f"K {K} column {k}: relative difference {rel:.3e}, r^2 {r2:.3e}")
        if k in (1, 2):
            assert rel <= r2, (k, rel, r2)
            if far:
                assert rel >= 0.02 * r2, (k, rel, r2)  # the neglected term is there, at its order
        else:
            assert rel <= 1e-8, (k, rel)


@pytest.mark.parametrize("frame,drift,K", [("az/el", False, 5), ("ra/dec", True, 5), ("ra/dec", False, 7), ("az/el", True, 7)])
def test_reference_fit_recovers_injected_parameters(frame, drift, K):
    """The numpy Levenberg-Marquardt on the reference's sums, from the nominal offsets and a 10 % wrong amplitude and
    width, recovers the parameters ``inject_source`` put in: the data are the model in float32, so the fit is within
    float32 rounding of the truth (1e-6 of every parameter's natural size).  The detector that never crosses the source
    fails with NaNs, alone."""
    case = R.make_case(frame, drift=drift, K=K)
    win = R.window_of(case)
    fit = R.lm_fit(lambda p: R.sums(case["x"], case["G"], p, win, None, case["src"]), R.start_of(case))
    assert fit["ok"][:-1].all() and not fit["ok"][-1] and np.isnan(fit["params"][-1]).all()
    err = np.abs(fit["params"][:-1] - case["truth"][:-1]) / R.scales(case["truth"][:-1])
    print(f"largest scaled error {err.max():.3e}")
    assert err.max() <= 1e-6


def test_fwhm_and_angle_from_known_quadratic_forms():
    import torch

    from maria_amd import beamfit

    rng = np.random.default_rng(1)
    sM, sm = rng.uniform(2e-4, 6e-4, 40), rng.uniform(5e-5, 2e-4, 40)
    th = rng.uniform(-np.pi / 2, np.pi / 2, 40)
    th[:3] = [0.0, np.pi / 2, -np.pi / 4]
    lM, lm = 1.0 / sM**2, 1.0 / sm**2
    a, b, cc = lM * np.cos(th) ** 2 + lm * np.sin(th) ** 2, np.cos(th) * np.sin(th) * (lM - lm), lM * np.sin(th) ** 2 + lm * np.cos(th) ** 2
    major, minor, angle = (z.numpy() for z in beamfit.shape_to_fwhm(*(torch.as_tensor(z) for z in (a, b, cc))))
    k = np.sqrt(8 * np.log(2))
    np.testing.assert_allclose(major, k * sM, rtol=1e-9)
    np.testing.assert_allclose(minor, k * sm, rtol=1e-9)
    want = np.where(th <= -np.pi / 2, th + np.pi, th)
    assert np.abs(np.angle(np.exp(2j * (angle - want)))).max() <= 1e-8  # (an axis: modulo pi)
    assert np.all((angle > -np.pi / 2) & (angle <= np.pi / 2))
    rm, rn, ra = R.fwhm_angle(a, b, cc)
    np.testing.assert_allclose(major, rm, rtol=1e-12)
    np.testing.assert_allclose(minor, rn, rtol=1e-12)
    # a round beam: both axes the same, no NaN; a form that is not positive definite: NaN
    major, minor, angle = beamfit.shape_to_fwhm(*(torch.tensor(z, dtype=torch.float64) for z in ([4.0, 1.0], [0.0, 2.0], [4.0, 1.0])))
    assert float(major[0]) == float(minor[0]) and abs(float(major[0]) - k / 2.0) <= 1e-15 and np.isfinite(float(angle[0]))
    assert all(np.isnan(float(z[1])) for z in (major, minor, angle))


def test_beamfit_offsets_and_relative_gain():
    import torch

    from maria_amd import beamfit

    D = 6
    nan = float("nan")
    ok = torch.tensor([True, True, False, True, True, True])
    amp = torch.tensor([1.0, 2.0, nan, 10.0, 30.0, 20.0], dtype=torch.float64)
    dx = torch.tensor([0.1, 0.2, nan, 0.4, 0.5, 0.6], dtype=torch.float64)
    nominal = torch.arange(2 * D, dtype=torch.float64).reshape(D, 2)
    z = torch.zeros(D, dtype=torch.float64)
    fit = beamfit.BeamFit(amp, dx, -dx, z, z, z, z, z, z, z.to(torch.int64), torch.zeros(D, 5, 5), z, z, ok, ok, torch.zeros(D, 5), nominal,
                          torch.tensor([0, 0, 0, 1, 1, 1]))
    off = fit.offsets()
    assert off.shape == (D, 2) and np.array_equal(off[2], [4.0, 5.0]) and np.array_equal(off[0], [0.1, -0.1])
    g = fit.relative_gain()
    np.testing.assert_allclose(g[[0, 1, 3, 4, 5]], [1 / 1.5, 2 / 1.5, 0.5, 1.5, 1.0])
    assert np.isnan(g[2])
    np.testing.assert_allclose(fit.relative_gain(None)[[0, 4]], [0.1, 3.0])
    with pytest.raises(ValueError):
        fit.relative_gain(np.zeros(3, np.int64))


def test_every_refusal_raises_before_a_device_call(monkeypatch):
    """Host tensors: everything the entries refuse is a ValueError, and valid arguments on the host are refused last,
    for not being on a device; no context is ever made."""
    import torch

    from maria_amd import beamfit

    def no_context(*a, **k):
        raise AssertionError("a device call was reached")

    monkeypatch.setattr(beamfit, "_context", no_context)
    D, T = 3, 40
    x = torch.zeros((D, T), dtype=torch.float32)
    point = dict(az=torch.zeros(T), el=torch.ones(T), transform=None, dx=torch.zeros(D), dy=torch.zeros(D))
    flags = torch.zeros((D, T), dtype=torch.uint8)
    center = (0.1, 0.2)
    params = torch.ones((D, 5), dtype=torch.float64)
    bad_flag_calls = [
        dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(value=0), dict(value=256), dict(value=1.5), dict(value=True),
        dict(center=(0.1,)), dict(center=(float("nan"), 0.0)), dict(center="x"), dict(src=np.zeros((T, 3))), dict(src=np.zeros((T + 1, 2))),
        dict(flags=torch.zeros((D, T + 1), dtype=torch.uint8)), dict(flags=torch.zeros((D, T), dtype=torch.float32)),
        dict(flags=torch.zeros((D, 2 * T), dtype=torch.uint8)[:, ::2]),
        dict(pointing=dict(point, el=torch.ones(T + 1))), dict(pointing=dict(point, az=torch.zeros(T, dtype=torch.float64))),
        dict(pointing=dict(point, dy=torch.zeros(D + 1))), dict(pointing=dict(point, transform=torch.zeros((T, 9), dtype=torch.float32))),
        dict(pointing=dict(point, transform=torch.zeros((T, 8), dtype=torch.float64))), dict(pointing=dict(point, dx=None)),
        dict(pointing=dict(point, az=None)),
    ]
    for kw in bad_flag_calls:
        args = dict(pointing=point, center=center, radius=0.01, flags=flags)
        args.update(kw)
        with pytest.raises(ValueError):
            beamfit.source_flags(**args)
    with pytest.raises(ValueError, match="device"):
        beamfit.source_flags(point, center, 0.01, flags=flags)
    with pytest.raises(ValueError, match="device"):
        beamfit.source_flags(point, center, 0.01)
    bad_normal_calls = [
        dict(x=torch.zeros((D, T), dtype=torch.float64)), dict(x=torch.zeros(T)), dict(x=torch.zeros((D, 2 * T))[:, ::2]),
        dict(params=torch.ones((D, 6), dtype=torch.float64)), dict(params=torch.ones((D + 1, 5), dtype=torch.float64)),
        dict(params=torch.ones((D, 5), dtype=torch.float32)), dict(flags=torch.zeros((D, T), dtype=torch.int32)),
        dict(flags=torch.zeros((D + 1, T), dtype=torch.uint8)), dict(model=torch.zeros((D, T), dtype=torch.float64)),
        dict(model=torch.zeros((D, T - 1))), dict(src=np.zeros((T, 1))), dict(center=(0.0, float("inf"))),
        dict(pointing=dict(point, el=torch.ones(T - 1))), dict(pointing=dict(point, transform=torch.zeros((T + 1, 9), dtype=torch.float64))),
    ]
    for kw in bad_normal_calls:
        args = dict(x=x, pointing=point, center=center, params=params, flags=flags)
        args.update(kw)
        with pytest.raises(ValueError):
            beamfit.normal_equations(**args)
    with pytest.raises(ValueError, match="device"):
        beamfit.normal_equations(x, point, center, params, flags=flags)
    # the nominal offsets are not read: a pointing without them is taken
    with pytest.raises(ValueError, match="device"):
        beamfit.normal_equations(x, dict(az=point["az"], el=point["el"]), center, torch.ones((D, 7), dtype=torch.float64))
    for kw in (dict(n_iter=0), dict(n_iter=2.5), dict(tol=0.0), dict(tol=float("nan")), dict(min_hits=-1), dict(rcond=1.0), dict(rcond=-0.1),
               dict(lam0=0.0), dict(flags=None), dict(init=torch.ones((D, 7), dtype=torch.float64)), dict(init=torch.ones((D, 4), dtype=torch.float64))):
        args = dict(x=x, pointing=point, center=center, init=params, flags=flags)
        args.update(kw)
        with pytest.raises(ValueError):
            beamfit.fit(**args)
    with pytest.raises(ValueError, match="device"):
        beamfit.fit(x, point, center, params, flags)
    with pytest.raises(ValueError):
        beamfit.inject_source(np.zeros((D, T)), np.zeros(T), np.zeros(T), None, center, np.ones((D, 6)))
    with pytest.raises(ValueError):
        beamfit.inject_source(np.zeros((D, T)), np.zeros(T + 1), np.zeros(T), None, center, np.ones((D, 5)))


def test_inject_source_is_the_reference_model():
    from maria_amd import beamfit

    case = R.make_case("ra/dec", drift=True, K=7, D=4)
    ox, oy = R.offsets(case["G"], *R.trial_offsets(case["truth"]))
    u, v = ox - case["src"][None, :, 0].astype(np.float64), oy - case["src"][None, :, 1].astype(np.float64)
    want = R.model(case["truth"], u, v)[0]
    assert np.abs(case["x"] - want).max() <= 2.0**-24 * np.abs(want).max()
    base = np.full(case["x"].shape, 0.25, np.float32)
    got = beamfit.inject_source(base, case["az"], case["el"], case["transform"], case["center"], case["truth"], src=case["src"])
    assert np.abs(got - (want + 0.25)).max() <= 2.0**-23 * np.abs(want + 0.25).max() and np.all(base == 0.25)


MARGIN = 4.0  # the kernel tests' acceptance in envelopes (test_gpu_beamfit.MARGIN)


def test_offaxis_builder_moves_the_array_and_the_centre():
    """``make_offaxis_case`` with nothing moved is ``make_case``'s geometry with the source at the array's mean; moved, the
    detectors still cross the source, which sits ``center_shift`` from the centre."""
    plain = R.make_case("ra/dec", drift=False, K=7)
    same = R.make_offaxis_case("ra/dec", K=7)
    assert set(same) == set(plain) and same["center"] == plain["center"] and np.array_equal(same["az"], plain["az"])
    assert np.array_equal(same["G"], plain["G"]) and np.array_equal(same["nominal"][:-1], plain["nominal"][:-1])
    assert same["src"].dtype == np.float32 and same["src"].shape == (same["T"], 2) and np.all(same["src"] == same["src"][0])
    assert np.hypot(*same["src"][0]) < np.radians(0.1)  # the array's mean over a daisy: near the scan's centre
    for number in (2, 6):
        case, flags, params = R.offaxis_case(number)
        make = R.OFFAXIS[number]["make"]
        assert set(case) == set(plain) and case["x"].dtype == np.float32 and case["x"].shape == (R.D_CASE, R.T_CASE)
        r = np.hypot(*case["src"].astype(np.float64).T)
        shift, common = make["center_shift"], np.hypot(*make.get("common", (0.0, 0.0)))
        assert np.all((r > abs(shift - common) - 0.01) & (r < shift + common + 0.01)), (r.min(), r.max())  # (a triangle on the sphere)
        assert (case["src"][-1] != case["src"][0]).all() == bool(make.get("drift"))
        hits = (R.window_of(case) == 0).sum(axis=1)
        assert hits.min() > 100 and case["x"].max() > 0.7  # every detector crosses the source
        assert np.abs(case["nominal"] - np.asarray(make.get("common", (0.0, 0.0))) - same["nominal"]).max() < 1e-15


@pytest.mark.parametrize("number", sorted(R.OFFAXIS))
def test_offaxis_cases_show_the_jacobian_terms(number):
    """What makes the kernel test of an off-axis case mean something: its samples lie in the branches DESIGN 3.31 names
    (``offaxis_geometry``), and the reference with the Jacobian's asin(r)/r factor set to 1 (cases 1, 2, 6) or its
    curvature term h set to 0 (cases 3 - 6) differs from the true one by more than 2 MARGIN envelopes in at least one
    entry of JtJ of EVERY row with hits: a kernel wrong in that term cannot pass.  For the flag test of cases 1 and 6:
    fewer than 1 % of the samples lie within MARGIN spacings (and within 6e-7 rad) of the radius."""
    case, flags, params = R.offaxis_case(number)
    print(R.offaxis_geometry(number))
    hits, _, JtJ, _ = R.sums(case["x"], case["G"], params, flags, None, case["src"])
    env = R.envelope(case["x"], case["G"], params, flags, None, case["src"])[1]
    live = hits > 0
    assert live.sum() == case["D"] - 1 and not live[3] and hits[live].min() > 100
    assert np.array_equal(R.mutant_JtJ(case["x"], case["G"], params, flags, case["src"]), JtJ)  # (no mutation: the reference itself)
    for name in R.OFFAXIS[number]["mutants"]:
        mutant = R.mutant_JtJ(case["x"], case["G"], params, flags, case["src"], **{name: True})
        ratio = (np.abs(mutant - JtJ)[live] / env[live]).reshape(int(live.sum()), -1).max(axis=1)
        print(f"case {number} {name}: |mutant - reference| / envelope, the rows' largest entries {ratio.min():.1f} .. {ratio.max():.1f}")
        assert ratio.min() > 2.0 * MARGIN, (name, float(ratio.min()))
    if number in (1, 6):
        dist = np.sqrt(case["dist2"])
        for radius in (R.RADIUS, 0.4 * R.RADIUS):
            assert (np.abs(dist - radius) <= 6e-7).mean() < 0.01 and 0.02 < (dist <= radius).mean() < 0.98


@pytest.mark.parametrize("frame,K,D,T", [("az/el", 5, 1, 1), ("ra/dec", 7, 17, 5), ("az/el", 7, 33, 1025), ("ra/dec", 5, 3, 32769)])
def test_hover_builder_keeps_every_sample_in_the_beam(frame, K, D, T):
    """``make_hover_case`` asserts its own property (exp(-q / 2) in [0.05, 1] for every sample of every row at the truth and
    at the trial point); here also that the sums of a single sample are of unit size and the source is in the data."""
    case = R.make_hover_case(frame, K, D, T)
    assert case["src"] is None and case["x"].shape == (D, T) and case["x"].dtype == np.float32 and np.isfinite(case["x"]).all()
    assert np.hypot(*case["nominal"].T).max() <= 0.2 * R.FWHM * (1 + 1e-12) and np.sqrt(case["dist2"].max()) < 1.0 * R.FWHM
    assert case["x"].min() >= -0.011 and case["x"].max() <= 1.26  # A g + c with A in 0.8 .. 1.2, g in 0.05 .. 1, |c| <= 0.05
    hits, chi2, JtJ, Jtr = R.sums(case["x"][:, :1], case["G"][:1], R.start_of(case))
    assert np.all(hits == 1) and np.all(JtJ[:, 0, 0] >= 0.05**2) and np.all(JtJ[:, -1, -1] == 1.0)


def test_seeded_flags_and_probe_positions():
    for D, T in ((17, 1), (17, 5), (17, 1025), (3, 32769)):
        f = R.seeded_flags(D, T, seed=T)
        assert f.shape == (D, T) and f.dtype == np.uint8 and set(np.unique(f)) <= {0, 1, 4, 128}
        assert (f == 0).any()
        if T >= 1025:
            frac = (f != 0).mean(axis=1)
            assert np.all((frac >= 0.3) & (frac < 0.5)) and set(np.unique(f)) == {0, 1, 4, 128}
            single = (f[:, 1:-1] != 0) & (f[:, :-2] == 0) & (f[:, 2:] == 0)
            assert single.sum() >= D  # isolated flags beside the runs
    seen = set()
    for rotate in (0, 7, 14, 3):
        flags, kept = R.probe_flags(rotate)
        assert flags.shape == (R.D_PROBE, R.T_PROBE) and np.array_equal((flags == 0).sum(axis=1), (kept >= 0).astype(int))
        assert np.all(kept[16:31] == -1) and kept[31] >= 0 and kept[32] >= 0 and np.all(kept[:16] >= 0)
        assert all(flags[d, kept[d]] == 0 for d in np.flatnonzero(kept >= 0))
        seen |= set(kept[kept >= 0].tolist())
    assert seen == set(R.PROBE_POSITIONS) and max(R.PROBE_POSITIONS) == R.T_PROBE - 1
    assert -(-R.T_PROBE // 1024) == 34 and -(-34 // 16) == 3  # 34 tiles in three chunks of 16, 16 and 2


def test_entries_are_declared_and_bound():
    from maria_amd import _lib

    header = open(os.path.join(ROOT, "include", "mrx.h")).read()
    for name, n_args in (("mrx_tod_source_flag", 16), ("mrx_tod_beam_normal", 23), ("mrx_tod_beam_normal_work_bytes", 4)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    makefile = open(os.path.join(ROOT, "maria_amd", "csrc", "Makefile")).read()
    assert "mrx_beamfit.hip" in makefile and "mrx_map_pointing.h" in makefile
    flags = dict(re.findall(r"^EXTRA_(\w+) := (.*)$", makefile, flags=re.M))
    assert flags["mrx_beamfit"] in ("$(EXTRA_mrx_map)", flags["mrx_map"])  # the binning's bits need the binning's flags
    # ... and so does the sampler, a translation unit of its own on the same pointing code
    assert "mrx_map_sample.hip" in makefile
    assert flags["mrx_map_sample"] in ("$(EXTRA_mrx_map)", flags["mrx_map"])
