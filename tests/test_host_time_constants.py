"""The host side of detector time constants (maria_amd.time_constants) without a GPU: the poles, every
Python-side refusal, the instrument tables carrying tau, the simulation's decision to leave an unlagged run alone, the
reference of tests/timeconst_ref.py against scipy, and the size of the mistakes the GPU test has to see."""

import numpy as np
import pytest
import timeconst_ref as ref

from maria_amd import time_constants


def test_poles_against_the_formula():
    tau = np.array([0.0, 1e-3, 5e-3, 0.2])
    a = time_constants.poles(tau, 200.0)
    assert a.dtype == np.float64 and a.shape == (4,) and a[0] == 0.0
    assert np.array_equal(a[1:], np.exp(-1.0 / (200.0 * tau[1:])))
    assert np.all((a >= 0) & (a < 1))
    assert time_constants.poles(0.005, 50.0).tolist() == [np.exp(-1.0 / 0.25)]
    assert time_constants.poles(1e-9, 50.0).tolist() == [0.0]  # exp underflows: no lag
    for bad in (-1e-3, np.nan, np.inf, [1e-3, -1e-3], [[1e-3]]):
        with pytest.raises(ValueError):
            time_constants.poles(bad, 50.0)
    for fs in (0.0, -50.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            time_constants.poles(1e-3, fs)
    t = 1.7e9 + np.arange(3000) / 50.0
    assert time_constants.sample_rate_of(t) == (t.size - 1) / (t[-1] - t[0])
    for bad in ([0.0], [1.0, 1.0], np.zeros((2, 2))):
        with pytest.raises(ValueError):
            time_constants.sample_rate_of(bad)


@pytest.mark.parametrize("fn", [time_constants.apply, time_constants.deconvolve])
def test_python_refusals(fn):
    """Every refusal before the device call, each with a message; a host tensor gets every other one first."""
    import torch

    x = torch.zeros((3, 40), dtype=torch.float32)
    a = np.array([0.0, 0.5, 0.9])
    for bad, msg in (
        (lambda: fn(x.numpy(), a), "float32 tensor"),
        (lambda: fn(x.double(), a), "float32 tensor"),
        (lambda: fn(x[0], a), "float32 tensor"),
        (lambda: fn(x[:, :0], a), "need D >= 1"),
        (lambda: fn(torch.zeros((3, 80))[:, ::2], a), "unit stride"),
        (lambda: fn(x, a[:2]), "one pole a row"),
        (lambda: fn(x, a.astype(np.float32)), "float64"),
        (lambda: fn(x, a[None]), "one pole a row"),
        (lambda: fn(x, torch.as_tensor(a[:2])), "one pole a row"),
        (lambda: fn(x, np.array([0.0, 1.0, 0.5])), r"in \[0, 1\)"),
        (lambda: fn(x, np.array([0.0, -0.1, 0.5])), r"in \[0, 1\)"),
        (lambda: fn(x, np.array([0.0, np.nan, 0.5])), r"in \[0, 1\)"),
        (lambda: fn(x, a, init="warm"), "steady"),
        (lambda: fn(x, a, init=1), "steady"),
        (lambda: fn(x, a, out=torch.zeros((3, 41))), "out must be"),
        (lambda: fn(x, a, out=torch.zeros((3, 40), dtype=torch.float64)), "out must be"),
        (lambda: fn(x, a, out=torch.zeros((3, 80))[:, ::2]), "unit stride"),
        (lambda: fn(x[:, :39], a, out=x[:, 1:]), "overlap"),
        (lambda: fn(x, a), "device tensor"),
        (lambda: fn(x, a, out=x), "device tensor"),
    ):
        with pytest.raises(ValueError, match=msg):
            bad()


def test_the_package_module_never_imports_the_oracle():
    import inspect
    import re

    assert not re.search(r"^\s*(from|import)\s+oracle\b", inspect.getsource(time_constants), flags=re.M)


def test_band_and_detectors_carry_the_time_constant():
    from maria_amd.instrument import Band, Detectors

    slow, fast, none = (Band(center=93e9, width=27e9, name="f093", time_constant=8e-3), Band(center=150e9, width=41e9, name="f150", time_constant=3e-3),
                        Band(center=220e9, width=40e9, name="f220"))
    assert (slow.time_constant, fast.time_constant, none.time_constant) == (8e-3, 3e-3, 0.0)
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError):
            Band(center=93e9, width=27e9, time_constant=bad)
    pos = np.zeros((5, 2))
    dets = Detectors(pos, [slow, fast, none], [0, 1, 2, 1, 0])
    assert dets.time_constant.tolist() == [8e-3, 3e-3, 0.0, 3e-3, 8e-3]  # None: each detector's band value
    assert Detectors(pos, [slow, fast, none], [0, 1, 2, 1, 0], time_constant=4e-3).time_constant.tolist() == [4e-3] * 5
    own = np.array([1e-3, 2e-3, 0.0, 4e-3, 5e-3])
    dets = Detectors(pos, [slow, fast, none], [0, 1, 2, 1, 0], time_constant=own)
    assert dets.time_constant.tolist() == own.tolist() and dets.time_constant is not own
    assert dets.subset([4, 1]).time_constant.tolist() == [5e-3, 2e-3]
    assert dets.subset(np.arange(1, 3)).time_constant.tolist() == [2e-3, 0.0]
    assert dets.one_detector_from_each_band().time_constant.tolist() == [1e-3, 2e-3, 0.0]
    for bad in (-1e-3, [1e-3] * 4, np.nan):
        with pytest.raises(ValueError):
            Detectors(pos, [slow, fast, none], [0, 1, 2, 1, 0], time_constant=bad)
    hexa = Detectors.hexagon(7, 0.5, [slow, fast])
    assert hexa.n == 14 and hexa.time_constant.tolist() == [8e-3] * 7 + [3e-3] * 7
    assert Detectors.hexagon(7, 0.5, [slow, fast], time_constant=1e-3).time_constant.tolist() == [1e-3] * 14
    assert Detectors.hexagon(7, 0.5, [slow, fast], time_constant=np.arange(14) * 1e-3).subset([13]).time_constant.tolist() == [13 * 1e-3]
    assert Detectors.hexagon(7, 0.5, [none]).time_constant.tolist() == [0.0] * 7


def test_a_simulation_without_time_constants_takes_the_old_path():
    """Where every tau of the rows is 0, run_obs applies nothing: the decision is ``Simulation._time_constants``, None for
    such rows (no launch, no metadata key, units as asked), the rows' tau otherwise, a shard's rows by themselves."""
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation

    plan = Plan.back_and_forth(duration=10.0)
    plain = [Band(center=93e9, width=27e9, name="f093"), Band(center=150e9, width=41e9, name="f150")]
    lagged = [Band(center=93e9, width=27e9, name="f093"), Band(center=150e9, width=41e9, name="f150", time_constant=3e-3)]
    for dets in (Detectors.hexagon(32, 0.5, plain), Detectors.hexagon(32, 0.5, plain, time_constant=0.0), Detectors.hexagon(32, 0.5, lagged, time_constant=0.0)):
        sim = Simulation(Instrument(dets), plan, Site(altitude=5000.0), noise=False)
        assert sim._time_constants(sim.instrument.dets) is None
    dets = Detectors.hexagon(32, 0.5, lagged)
    sim = Simulation(Instrument(dets), plan, Site(altitude=5000.0), noise=False, shard=(0, 2))
    assert sim._time_constants(dets).tolist() == [0.0] * 32 + [3e-3] * 32
    lo, hi = sim._rows(dets.n)
    assert (lo, hi) == (0, 32) and sim._time_constants(dets.subset(np.arange(lo, hi))) is None  # this shard's rows have no lag
    assert sim._time_constants(dets.subset(np.arange(32, 64))).tolist() == [3e-3] * 32


def test_tod_deconvolve_refuses_before_any_device_call():
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    T = 50
    dets = Detectors(np.zeros((3, 2)), [Band(center=150e9, width=30e9, name="f150", time_constant=3e-3)])
    coords = Coordinates(np.arange(T) / 50.0, np.zeros(T), np.full(T, 1.0))
    tod = TOD({"signal": np.zeros((3, T), np.float32)}, dets, coords, metadata={"downsample": {"factor": 2}})
    with pytest.raises(NotImplementedError, match="deconvolve first"):
        tod.deconvolve_time_constants()
    tod = TOD({"signal": np.zeros((3, T), np.float32)}, dets, coords)
    for kw in (dict(init="warm"), dict(tau=-1e-3), dict(tau=[1e-3, 2e-3]), dict(tau=np.nan), dict(tau=np.zeros((3, 1)))):
        with pytest.raises(ValueError):
            tod.deconvolve_time_constants(**kw)


@pytest.mark.parametrize("init", [0, 1])
def test_the_reference_is_scipy_lfilter(init):
    """forward64 against scipy.signal.lfilter([g], [1, -a], x, zi): zi = a x[0] is the steady state (lfilter then forms
    g x[0] + a x[0], one rounding from x[0]), no zi the zero state.  Equal to float64 rounding: a few ulp of the largest
    value.  The inverse undoes it to the round-trip bound."""
    import scipy.signal

    for D, T in ((3, 5), (33, 1025), (3, 4099)):
        x, a = ref.case(D, T)
        y = ref.case_forward64(D, T, init)
        assert y.dtype == np.float64 and y.shape == (D, T)
        for d in range(D):
            x64 = x[d].astype(np.float64)
            if not ref.lagged(a[d]):
                assert np.array_equal(y[d], x64)
                continue
            g = 1.0 - a[d]
            want, _ = scipy.signal.lfilter([g], [1.0, -a[d]], x64, zi=[a[d] * x64[0] if init else 0.0])
            assert np.abs(want - y[d]).max() <= 4 * 2.0**-53 * np.abs(y[d]).max(), (D, T, d)
        stored = y.astype(np.float32)
        back = ref.inverse(stored, a, init)
        assert back.dtype == np.float32 and np.all(np.abs(back.astype(np.float64) - x) <= ref.round_trip_bound(x, stored, a))
        assert np.array_equal(back[~ref.lagged(a)], x[~ref.lagged(a)])


def test_the_cases_mix_every_pole():
    seen = set()
    for D in ref.ROWS:
        for T in ref.TIMES:
            x, a = ref.case(D, T)
            assert x.shape == (D, T) and x.dtype == np.float32 and a.shape == (D,) and set(a.tolist()) <= set(ref.POLES)
            assert T < 2 or x[D - 1].max() > 9e5
            assert T < ref.TILE - 1 or a[0] == 1.0 - 2.0**-12
            seen |= set(a.tolist())
    assert seen == set(ref.POLES)
    assert len({tuple(ref.case(33, T)[1].tolist()) for T in ref.TIMES}) > 10  # in a random order


@pytest.mark.parametrize("init", [0, 1])
def test_the_bound_holds_for_a_float64_scan_and_sees_the_mistakes(init):
    """The size of the mistakes, on the GPU test's own rows at a = 1 - 2^-12 (the first row of its cases that have more
    than one tile), the worst sample of all of them.

    A blocked scan in float64 (tiles of 1024, the powers from numpy's own pow: another association order than the
    kernel's) stays inside the forward bound 2^-24 |y64| + 64 2^-53 max|x| / (1 - a) once stored as float32, and inside
    its float64 term alone before the store (measured: 5e-5 of that term).

    A carry dropped at one seam exceeds the whole bound by more than 100 x in every case (measured: 1.7e7 x).

    A float32 carry makes an error of up to 2^-24 |y64| of the carry.  That is the size of the bound's own first term,
    the float32 store, so it cannot exceed the whole bound by 100 x.  The factor 100 holds against the float64 term, which
    is what the scan's float64 results are held to (measured: 290 x and 810 x).  Once stored as float32 its worst sample
    of all the cases is at 1.6 .. 1.9 x the whole bound (printed, not asserted: in single cases it stays inside, 0.98 x): a
    GPU test that checks every sample of every case against the whole bound is likely, not sure, to see it."""
    a0 = 1.0 - 2.0**-12
    worst = {"float64": 0.0, "float32 carry": 0.0, "float32 carry, stored": 0.0, "dropped carry": np.inf}
    for T in [T for T in ref.TIMES if T > ref.TILE]:
        x, a = ref.case(3, T)
        assert a[0] == a0
        y64 = ref.case_forward64(3, T, init)[:1]
        whole, term = ref.forward_bound(y64, x[:1], a[:1])[0], float(ref.float64_term(x[:1], a[:1])[0, 0])
        stored = lambda y: np.abs(y.astype(np.float32).astype(np.float64) - y64[0])  # noqa: E731
        good = ref.blocked_scan(x[0], a0, init)
        assert np.all(stored(good) <= whole) and np.all(np.abs(good - y64[0]) <= term)
        worst["float64"] = max(worst["float64"], float(np.abs(good - y64[0]).max() / term))
        f32 = ref.blocked_scan(x[0], a0, init, carry_dtype=np.float32)
        worst["float32 carry"] = max(worst["float32 carry"], float(np.abs(f32 - y64[0]).max() / term))
        worst["float32 carry, stored"] = max(worst["float32 carry, stored"], float((stored(f32) / whole).max()))
        lost = ref.blocked_scan(x[0], a0, init, drop_seam=(T - 1) // ref.TILE)
        worst["dropped carry"] = min(worst["dropped carry"], float((stored(lost) / whole).max()))
    print(f"init {init}: error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst["float32 carry"] >= 100.0
    assert worst["dropped carry"] >= 100.0
