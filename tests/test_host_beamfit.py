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
