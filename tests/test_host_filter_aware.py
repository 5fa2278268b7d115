"""The filter-aware map's host side (no GPU needed): the float64 restatement of F and F^T that the GPU tests lean on is
its own adjoint pair, and MaximumLikelihoodMapper's ``filter_aware`` keyword is checked at construction."""

import numpy as np
import pytest

import filter_aware_ref as ref

FULL = {"remove_slope": {}, "remove_spline": {"knot_spacing": 15.0, "remove_el_gradient": True}, "window": {"name": "hann"},
        "filter": {"f_lower": 0.2, "f_upper": 10.0}, "remove_modes": {"modes_to_remove": 2}}


def _tod(n=6, T=50):
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    dets = Detectors(np.zeros((n, 2)), [Band(center=150e9, width=30e9, name="f150")])
    t = np.arange(T) / 50.0
    return TOD({"map": np.zeros((n, T), np.float32)}, dets, Coordinates(t, np.zeros(T), np.full(T, 1.0), offsets=dets.offsets), units="K_RJ")


@pytest.mark.parametrize("T", [2, 3, 257, 3000])
def test_reference_adjoint_identity(T):
    """<F x, y> = <x, F^T y> to 1e-10 of |F x| |y| for the five-step config (T >= 257; the short rows take the steps
    that exist there: slope, window, filter, modes)."""
    rng = np.random.default_rng(T)
    D = 12
    t = 1.7e9 + np.arange(T) / 50.0
    el = 0.9 + 0.01 * np.sin(np.arange(T) / 300.0) + 1e-4 * np.arange(T) / max(T, 1)
    config = dict(FULL) if T >= 257 else {k: v for k, v in FULL.items() if k != "remove_spline"}
    U = np.linalg.qr(rng.normal(size=(D, 2)))[0]
    steps = ref.build(config, t, el, modes=(U, rng.uniform(0.5, 20.0, D)))
    assert [name for name, _ in steps] == [k for k in ("remove_slope", "remove_spline", "window", "filter", "remove_modes") if k in config]
    for _ in range(3):
        x, y = np.cumsum(rng.normal(size=(D, T)), axis=1) + 30.0, rng.normal(size=(D, T))
        Fx, Fty = ref.apply(steps, x), ref.apply_transpose(steps, y)
        lhs, rhs = np.sum(Fx * y), np.sum(x * Fty)
        scale = np.linalg.norm(Fx) * np.linalg.norm(y) + np.linalg.norm(x) * np.linalg.norm(Fty)
        assert abs(lhs - rhs) <= 1e-10 * max(scale, 1e-300), (lhs, rhs, scale)


def test_slope_transpose_is_the_matrix_transpose():
    T = 7
    M = np.stack([ref.slope(e[None])[0] for e in np.eye(T)], axis=1)   # M[:, j] = S e_j
    Mt = np.stack([ref.slope_transpose(e[None])[0] for e in np.eye(T)], axis=1)
    np.testing.assert_allclose(Mt, M.T, atol=1e-15)


def test_filter_aware_refusals():
    """filter_aware with noise_model (or noise_modes), and a value that is not a bool: ValueError at construction."""
    from maria_amd.mappers import MaximumLikelihoodMapper

    kw = dict(center=(0.0, 0.0), width=1.0, resolution=0.1, frame="az/el")
    ok = MaximumLikelihoodMapper([_tod()], filter_aware=True, tod_preprocessing={"filter": {"f_lower": 0.2}}, **kw)
    assert ok.filter_aware is True
    assert MaximumLikelihoodMapper([_tod()], **kw).filter_aware is False
    with pytest.raises(ValueError, match="filter_aware"):
        MaximumLikelihoodMapper([_tod()], filter_aware=True, noise_model="fit", **kw)
    with pytest.raises(ValueError, match="filter_aware"):
        MaximumLikelihoodMapper([_tod()], filter_aware=True, noise_model={"white": 1e-4, "knee": 1.0, "alpha": 1.0}, **kw)
    with pytest.raises(ValueError, match="filter_aware"):
        MaximumLikelihoodMapper([_tod()], filter_aware=True, noise_model="fit", noise_modes=2, **kw)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="filter_aware"):
            MaximumLikelihoodMapper([_tod()], filter_aware=bad, **kw)


def test_new_entry_points_are_bound():
    from maria_amd import _lib

    lib = _lib.load()
    assert _lib.SIGNATURES["mrx_sosfilt_transpose"] == _lib.SIGNATURES["mrx_sosfilt"]
    for name in ("mrx_sosfilt_transpose", "mrx_tod_detrend_window_transpose"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
