"""CPU tier of maria_amd.regress: the two forms of the numpy reference agree; ``solve`` (torch on the host)
against numpy's least squares; the Legendre and airmass templates; every Python-side refusal on host tensors, before any
device call; the conditioning of the templates the device tests use."""

import numpy as np
import pytest
import regress_ref as ref

from maria_amd import regress


def templates(G, K, T, seed):
    """[G, K, T] float32: P_0 .. P_3 of the time axis, then Gaussian rows (what tests/test_gpu_regress.py fits)."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((G, K, T)).astype(np.float32)
    n = min(K, 4)
    B[:, :n, :] = regress.legendre_templates(T, 3)[None, :n]
    return B


def case(D, T, G, K, seed, exact):
    rng = np.random.default_rng(seed)
    if exact:
        x = rng.integers(-64, 65, (D, T)).astype(np.float32)
        model = rng.integers(-16, 17, (D, T)).astype(np.float32)
        B = rng.integers(-4, 5, (G, K, T)).astype(np.float32)
        u, v, off = (rng.integers(0, 5, D).astype(np.float64) for _ in range(3))
    else:
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        model = rng.standard_normal((D, T)).astype(np.float32)
        B = templates(G, K, T, seed + 1)
        u, v, off = rng.uniform(0.5, 2, D), rng.uniform(0.5, 2, D), rng.standard_normal(D)
    flags = ((rng.random((D, T)) < 0.1) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    groups = rng.integers(-1, G, D).astype(np.int32)
    return x, model, flags, groups, B, u, v, off


@pytest.mark.parametrize("exact", [True, False])
def test_the_two_forms_of_the_reference_agree(exact):
    for D, T, G, K, with_flags, with_model, with_off in ((5, 17, 2, 3, True, True, True), (1, 1, 1, 1, False, False, False),
                                                         (7, 33, 3, 8, True, False, True), (4, 9, 1, 2, False, True, False)):
        x, model, flags, groups, B, u, v, off = case(D, T, G, K, 100 * D + T, exact)
        kw = dict(groups=groups, flags=flags if with_flags else None, model=model if with_model else None)
        S, W, mean, A = ref.column_mean(x, u, v, off=off if with_off else None, n_groups=G, **kw)
        S2, W2, mean2 = ref.column_mean_by_loops(x, u, v, off=off if with_off else None, n_groups=G, **kw)
        N, r, hits, aN, ar = ref.normal_equations(x, B, **kw)
        N2, r2, hits2 = ref.normal_equations_by_loops(x, B, **kw)
        assert np.array_equal(hits, hits2) and np.array_equal(W, W2)
        assert np.array_equal(S, S2) and np.array_equal(mean, mean2)  # both add the rows in ascending order
        if exact:
            assert np.array_equal(N, N2) and np.array_equal(r, r2)
        else:
            assert np.all(np.abs(N - N2) <= T * 2.0**-52 * aN) and np.all(np.abs(r - r2) <= T * 2.0**-52 * ar)
        assert np.array_equal(N, N.transpose(0, 2, 1)) and not N[(groups < 0)].any() and not hits[groups < 0].any()


def test_apply_reference_by_hand():
    x = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], np.float32)
    B = np.array([[[1.0, 1.0, 1.0], [0.0, 1.0, 2.0]]], np.float32)
    a = np.array([[0.5, 2.0], [9.0, 9.0]])
    y = ref.apply(x, B, a, groups=np.array([0, -1]), sign=-1)
    assert np.array_equal(y, np.array([[0.5, -0.5, -1.5], [4.0, 5.0, 6.0]], np.float32))
    assert np.array_equal(ref.apply(y, B, a, groups=np.array([0, -1]), sign=+1), x)


def test_the_test_templates_are_well_conditioned():
    """The diagonally scaled N of P_0 .. P_3 and Gaussian rows under 3 % flags: condition <= 1e3 at every length the
    device tests solve at (the bound their tolerance is built on)."""
    worst = 0.0
    for T in (16, 63, 64, 65, 1023, 1025, 4099):
        for K in range(1, 9):
            if T < 4 * K:
                continue
            B = templates(1, K, T, 7 * T + K)
            flags = (np.random.default_rng(T + K).random((3, T)) < 0.03).astype(np.uint8)
            N, _, _, _, _ = ref.normal_equations(np.zeros((3, T), np.float32), B, flags=flags)
            for d in range(3):
                s = 1.0 / np.sqrt(np.diagonal(N[d]))
                worst = max(worst, np.linalg.cond(N[d] * s[:, None] * s[None, :]))
    print(f"largest condition number of a scaled N: {worst:.1f}")
    assert worst <= 1e3


def test_solve_against_lstsq():
    import torch

    D, T, K = 6, 257, 5
    x, _, flags, _, _, _, _, _ = case(D, T, 1, K, 3, exact=False)
    B = templates(1, K, T, 4)
    flags[4, :] = 1  # wholly flagged
    flags[5, : T - 3] = 1  # fewer samples than templates
    N, r, hits, _, _ = ref.normal_equations(x, B, flags=flags)
    a_ref, ok_ref = ref.solve(N, r, hits, min_hits=1)
    a, ok = regress.solve(torch.as_tensor(N), torch.as_tensor(r), torch.as_tensor(hits), min_hits=1)
    a, ok = a.numpy(), ok.numpy()
    assert ok.tolist() == ok_ref.tolist() == [True, True, True, True, False, False]
    assert not a[4:].any() and not a_ref[4:].any()
    for d in range(4):
        keep = flags[d] == 0
        want = np.linalg.lstsq(B[0][:, keep].astype(np.float64).T, x[d, keep].astype(np.float64), rcond=None)[0]
        scale = np.abs(want).max()
        assert np.abs(a[d] - want).max() <= 1e-10 * scale and np.abs(a_ref[d] - want).max() <= 1e-10 * scale
    # min_hits, a duplicated template and a zero template
    assert not regress.solve(torch.as_tensor(N), torch.as_tensor(r), torch.as_tensor(hits), min_hits=10**6)[1].any()
    dup = B.copy()
    dup[0, 3] = dup[0, 1]
    zero = B.copy()
    zero[0, 2] = 0
    for bad in (dup, zero):
        N, r, hits, _, _ = ref.normal_equations(x[:2], bad)
        a, ok = regress.solve(torch.as_tensor(N), torch.as_tensor(r), torch.as_tensor(hits))
        assert not ok.any() and not a.numpy().any() and not ref.solve(N, r, hits)[1].any()


def test_legendre_and_airmass_templates():
    from numpy.polynomial import legendre

    for T in (1, 2, 17, 1000):
        for order in (0, 1, 5, 7):
            P = regress.legendre_templates(T, order)
            assert P.dtype == np.float32 and P.shape == (order + 1, T)
            want = legendre.legvander(np.linspace(-1.0, 1.0, T), order).T
            assert np.abs(P.astype(np.float64) - want).max() <= 2.0**-24 + 1e-14
    el = np.radians(np.linspace(40.0, 60.0, 101))
    a = regress.airmass_template(el)
    want = 1 / np.sin(el) - np.mean(1 / np.sin(el))
    assert a.dtype == np.float32 and np.abs(a - want).max() <= 2.0**-24 and abs(float(a.astype(np.float64).mean())) < 1e-7
    for bad in (lambda: regress.legendre_templates(0, 1), lambda: regress.legendre_templates(5, 8), lambda: regress.legendre_templates(5, -1),
                lambda: regress.airmass_template(np.array([0.0, 1.0])), lambda: regress.airmass_template(np.zeros((2, 2)) + 1),
                lambda: regress.airmass_template(np.array([np.nan]))):
        with pytest.raises(ValueError):
            bad()


def test_reference_fit_recovers_what_was_injected():
    """x = g_d c_t + o_d exactly representable: the reference fit returns the gains (normalised to mean 1) and offsets."""
    rng = np.random.default_rng(5)
    D, T = 6, 64
    c = rng.integers(-8, 9, T).astype(np.float64)
    gains = np.array([0.5, 0.75, 1.0, 1.0, 1.25, 1.5])
    offsets = rng.integers(-4, 5, D).astype(np.float64)
    x = (gains[:, None] * c[None, :] + offsets[:, None]).astype(np.float32)
    cm, a, g, ok, B = ref.fit_common_mode(x, n_iter=3, min_hits=1)
    assert ok.all() and B.shape == (1, 2, T) and np.array_equal(B[0, 1], cm[0])
    assert np.abs(g - gains).max() <= 1e-6 and abs(g.mean() - 1) <= 1e-12
    assert np.abs(ref.apply(x, B, a)).max() <= 8 * 2.0**-24 * np.abs(x).max()


def test_python_refusals_come_before_any_device_call():
    """Host tensors: every refusal of the C entries raises ValueError in Python, and a valid call raises at the last
    check, "x must be a device tensor", without touching a device."""
    import torch

    D, T, G, K = 4, 32, 2, 3
    x = torch.zeros((D, T), dtype=torch.float32)
    u = torch.ones(D, dtype=torch.float64)
    B = torch.ones((G, K, T), dtype=torch.float32)
    a = torch.zeros((D, K), dtype=torch.float64)
    flags = torch.zeros((D, T), dtype=torch.uint8)
    groups = np.array([0, 1, -1, 0], np.int32)
    last = "x must be a device tensor"
    with pytest.raises(ValueError, match=last):
        regress.column_mean(x, u, u, off=u, groups=groups, n_groups=G, flags=flags, model=x)
    with pytest.raises(ValueError, match=last):
        regress.normal_equations(x, B, groups=groups, flags=flags, model=x)
    with pytest.raises(ValueError, match=last):
        regress.apply(x, B, a, groups=groups)
    with pytest.raises(ValueError, match=last):
        regress.fit_common_mode(x, groups=groups, n_groups=G, flags=flags, model=x, extra=np.ones((2, T), np.float32))
    bad = [
        lambda: regress.column_mean(x.double(), u, u), lambda: regress.column_mean(x[:0], u[:0], u[:0]), lambda: regress.column_mean(x[:, ::2], u, u),
        lambda: regress.column_mean(x, u, u, n_groups=0), lambda: regress.column_mean(x, u, u, n_groups=17), lambda: regress.column_mean(x, u.float(), u),
        lambda: regress.column_mean(x, u, u[:3]), lambda: regress.column_mean(x, u, u, off=u[:3]), lambda: regress.column_mean(x, u, u, groups=groups[:3]),
        lambda: regress.column_mean(x, u, u, groups=groups.astype(np.float64)), lambda: regress.column_mean(x, u, u, flags=flags[:, :5]),
        lambda: regress.column_mean(x, u, u, flags=flags.float()), lambda: regress.column_mean(x, u, u, model=x[:2]),
        lambda: regress.normal_equations(x, B[0]), lambda: regress.normal_equations(x, B.double()), lambda: regress.normal_equations(x, B[:, :, :5]),
        lambda: regress.normal_equations(x, torch.ones((G, 9, T))), lambda: regress.normal_equations(x, torch.ones((17, 1, T))),
        lambda: regress.normal_equations(x, torch.ones((G, K + 1, T))[:, :K]),  # the groups are not K row pitches apart
        lambda: regress.normal_equations(x, torch.ones((G, K, 2 * T))[:, :, ::2]), lambda: regress.normal_equations(x, B, groups=groups[:2]),
        lambda: regress.normal_equations(x, B, flags=flags[:2]), lambda: regress.normal_equations(x, B, model=x.double()),
        lambda: regress.apply(x, B, a, sign=0), lambda: regress.apply(x, B, a, sign=2), lambda: regress.apply(x, B, a[:, :2]),
        lambda: regress.apply(x, B, a.float()), lambda: regress.apply(x, B, a, out=torch.zeros((D, T + 1))),
        lambda: regress.apply(x, B, a, out=torch.zeros((D, T), dtype=torch.float64)),
        lambda: regress.solve(torch.zeros((D, K, K)), torch.zeros((D, K)), torch.zeros(D, dtype=torch.int64)),
        lambda: regress.solve(torch.zeros((D, K, K), dtype=torch.float64), torch.zeros((D, 2), dtype=torch.float64), torch.zeros(D, dtype=torch.int64)),
        lambda: regress.solve(torch.zeros((D, K, K), dtype=torch.float64), torch.zeros((D, K), dtype=torch.float64), torch.zeros(D, dtype=torch.float64)),
        lambda: regress.solve(torch.zeros((D, K, K), dtype=torch.float64), torch.zeros((D, K), dtype=torch.float64), torch.zeros(D, dtype=torch.int64), min_hits=-1),
        lambda: regress.solve(torch.zeros((D, K, K), dtype=torch.float64), torch.zeros((D, K), dtype=torch.float64), torch.zeros(D, dtype=torch.int64), rcond=1.0),
        lambda: regress.fit_common_mode(x, n_iter=0), lambda: regress.fit_common_mode(x, n_groups=17), lambda: regress.fit_common_mode(x, min_hits=-1),
        lambda: regress.fit_common_mode(x, extra=np.ones((7, T), np.float32)), lambda: regress.fit_common_mode(x, extra=np.ones((1, T + 1), np.float32)),
        lambda: regress.fit_common_mode(x, extra=np.ones((1, T))), lambda: regress.fit_common_mode(x, groups=groups[:3]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError) as err:
            call()
        assert last not in str(err.value), f"refusal {i} got as far as the device check"
    # an output that overlaps x without being x
    buf = torch.zeros(D * T + 8, dtype=torch.float32)
    xv, yv = torch.as_strided(buf, (D, T), (T, 1), 0), torch.as_strided(buf, (D, T), (T, 1), 4)
    with pytest.raises(ValueError, match="overlap"):
        regress.apply(xv, B, a, out=yv)


def test_tod_method_refusals():
    from maria_amd.sim import TOD, Coordinates

    T = 16
    coords = Coordinates(np.arange(T) / 10.0, np.zeros(T), np.full(T, 1.0))
    tod = TOD({"a": np.zeros((3, T), np.float32)}, dets=None, coords=coords)
    for bad in (lambda: tod.regress(np.ones((9, T), np.float32)), lambda: tod.regress(np.ones((2, T + 1), np.float32)), lambda: tod.regress(np.ones(T, np.float32)),
                lambda: tod.regress(np.ones((1, T), np.float32), min_hits=-1), lambda: tod.regress(np.ones((1, T), np.float32), into="b"),
                lambda: tod.remove_common_mode(groups="row"), lambda: tod.remove_common_mode(groups=np.array([0, 17, 0])),
                lambda: tod.remove_common_mode(groups=np.array([0, -2, 0])), lambda: tod.remove_common_mode(groups=None, poly_order=7),
                lambda: tod.remove_common_mode(groups=None, poly_order=6, airmass=True), lambda: tod.remove_common_mode(groups=None, poly_order=-1),
                lambda: tod.remove_common_mode(groups=None, into="b"), lambda: tod.remove_common_mode(groups=None, min_hits=0.5)):
        with pytest.raises(ValueError):
            bad()
