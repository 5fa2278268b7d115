"""mrx_gauss_smooth2d / mrx_map_smooth on every launch route of csrc/mrx_gauss.hip, against scipy: interior tiles of the x
pass (directly and through the transposed plane), the four y-pass instances, the largest radii and the refusals past
them, radius 0, truncate != 4, the tap cache's wrap and eviction, and non-finite input.  The cases and the restatement
of the dispatch that says which branch each one reaches are in tests/gauss_cases.py (checked without a GPU by
tests/test_host_gauss_cases.py).  Bounds: max|got - ref| / max(1, max|ref|) <= 2.5e-7 in the exact mode, <= 1e-6 in the
blocked and default modes."""

import numpy as np
import pytest

import gauss_cases as gc

pytestmark = pytest.mark.gpu


def _smooth(ctx, a, sy, sx, truncate=4.0, inplace=False):
    import torch

    from maria_amd._lib import ptr

    d_in = torch.as_tensor(np.ascontiguousarray(a, np.float32)).to("cuda:0")
    d_out = d_in if inplace else torch.empty_like(d_in)
    d_tmp = torch.empty_like(d_in)
    ny, nx = a.shape
    ctx.call("mrx_gauss_smooth2d", ptr(d_in), ptr(d_out), ptr(d_tmp), ny, nx, float(sy), float(sx), float(truncate))
    return d_out.cpu().numpy()


class _mode:
    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        from maria_amd import _lib

        self.ctx.set_option(_lib.OPT_GAUSS_ACCUM, self.mode)

    def __exit__(self, *exc):
        from maria_amd import _lib

        self.ctx.set_option(_lib.OPT_GAUSS_ACCUM, 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _err(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("case", gc.cases("finite"), ids=lambda c: c["name"])
def test_finite_case_matches_scipy(gpu_ctx, case):
    """Every finite case of the table in each of its modes, out of place and (where the case says so) in place.
    The y pass's four-rows-a-thread instance (`y_rows4_r232`, `max_ry`) runs rim tiles only: an interior tile of it needs
    16 + 2 * 229 rows inside a plane wider than 262 140 columns, about 500 rows -- 0.5 GB and a minute of scipy -- and is
    left out."""
    a = gc.case_input(case["shape"])
    ref = gc.case_reference(case)
    small = all(r is None or r < 16 for r in (gc.case_plan(case).ry, gc.case_plan(case).rx))
    for mode in case["modes"]:
        with _mode(gpu_ctx, mode):
            got = _smooth(gpu_ctx, a, case["sy"], case["sx"], case["truncate"])
            got2 = _smooth(gpu_ctx, a, case["sy"], case["sx"], case["truncate"], inplace=True) if case["inplace"] else got
        err = _err(got, ref)
        print(f"{case['name']} mode {mode}: {err:.3e}")
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert err <= gc.BOUND[mode], (case["name"], mode, err)
        assert np.array_equal(_bits(got), _bits(got2))
        if mode == 0 and small:
            assert err <= gc.BOUND[1]  # (small stencils keep the exact arithmetic by default)


@pytest.mark.parametrize("case", gc.cases("refuse"), ids=lambda c: c["name"])
def test_one_radius_past_the_largest_is_refused(gpu_ctx, case):
    """MRX_ERR_UNSUPPORTED before any launch: the output keeps its sentinel."""
    import torch

    from maria_amd._lib import MrxError, ptr

    ny, nx = case["shape"]
    d_in = torch.zeros((ny, nx), dtype=torch.float32, device="cuda:0")
    d_out = torch.full((ny, nx), -7.5, dtype=torch.float32, device="cuda:0")
    d_tmp = torch.empty_like(d_in)
    with pytest.raises(MrxError) as e:
        gpu_ctx.call("mrx_gauss_smooth2d", ptr(d_in), ptr(d_out), ptr(d_tmp), ny, nx, case["sy"], case["sx"], case["truncate"])
    assert e.value.code == -4 and "exceeds the LDS tile" in str(e.value)
    axis = gc.case_plan(case).refused
    assert f"along {axis}" in str(e.value)
    torch.cuda.synchronize()
    assert bool((d_out == -7.5).all())


@pytest.mark.parametrize("case", gc.cases("bits"), ids=lambda c: c["name"])
def test_radius_zero_is_the_identity(gpu_ctx, case):
    """0 < sigma < 0.125: one tap of weight 1 -- the input's bits, in every mode, in place too."""
    a = gc.case_input(case["shape"])
    assert np.array_equal(gc.case_reference(case), a)  # scipy's too
    for mode in case["modes"]:
        with _mode(gpu_ctx, mode):
            for inplace in (False, True):
                got = _smooth(gpu_ctx, a, case["sy"], case["sx"], case["truncate"], inplace=inplace)
                assert np.array_equal(_bits(got), _bits(a)), (case["name"], mode, inplace)


def test_tap_cache_wraps_evicts_and_keys_on_truncate():
    """40 distinct sigmas through the 32 slots of a context of its own, the first (evicted) again, one sigma under
    truncate 3, 4, 3: every result against scipy, and bit for bit what a context that has never cached a tap gives."""
    import torch

    from maria_amd import Context

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    case = gc.BY_NAME["tap_cache"]
    a = gc.case_input(case["shape"])

    def context():
        c = Context(0)
        c.set_stream(torch.cuda.current_stream())
        return c

    ctx = context()
    try:
        for i, (sigma, truncate) in enumerate(case["calls"]):
            got = _smooth(ctx, a, 0.0, sigma, truncate)
            ref = gc.reference(a, 0.0, sigma, truncate)
            r = gc.radius_of(sigma, truncate)
            assert _err(got, ref) <= (gc.BOUND[1] if r < 16 else gc.BOUND[0]), (i, sigma, truncate)
            fresh = context()
            try:
                want = _smooth(fresh, a, 0.0, sigma, truncate)
            finally:
                fresh.close()
            assert np.array_equal(_bits(got), _bits(want)), (i, sigma, truncate)
    finally:
        ctx.close()


def _check_nonfinite(got, ref, bound, tag, bad):
    """isnan sets equal, isinf sets equal with their signs, the finite remainder inside the bound; collects into bad."""
    nan_extra, nan_missing = int((np.isnan(got) & ~np.isnan(ref)).sum()), int((~np.isnan(got) & np.isnan(ref)).sum())
    pinf = int(((got == np.inf) != (ref == np.inf)).sum())
    ninf = int(((got == -np.inf) != (ref == -np.inf)).sum())
    fin = np.isfinite(got) & np.isfinite(ref)
    scale = max(1.0, float(np.abs(ref[np.isfinite(ref)]).max()))
    err = float(np.abs(got[fin].astype(np.float64) - ref[fin]).max() / scale) if fin.any() else 0.0
    if nan_extra or nan_missing or pinf or ninf or not err <= bound:
        bad.append((tag, dict(nan_outside_ref=nan_extra, nan_missing=nan_missing, pinf_differ=pinf, ninf_differ=ninf, err=err)))
    return nan_extra


@pytest.mark.parametrize("case", gc.cases("nonfinite"), ids=lambda c: c["name"])
def test_nonfinite_pixel_spreads_as_in_scipy(gpu_ctx, case):
    """One NaN, +Inf or -Inf: scipy makes the pixels of its window, +-radius per filtered axis, non-finite and no others.
    The kernels' sliding windows give every staged value to all of a thread's outputs; where it is outside an output's
    window it must not meet that accumulator at all (a zero tap would make 0 * NaN = NaN)."""
    bad = []
    outside = {m: 0 for m in case["modes"]}
    for pixel in case["pixels"]:
        for value in gc.NONFINITE_VALUES:
            a = gc.nonfinite_input(case, pixel, value)
            ref = gc.reference(a, case["sy"], case["sx"], case["truncate"])
            assert not np.isfinite(ref).all()
            for mode in case["modes"]:
                with _mode(gpu_ctx, mode):
                    got = _smooth(gpu_ctx, a, case["sy"], case["sx"], case["truncate"])
                outside[mode] += _check_nonfinite(got, ref, gc.BOUND[mode], (pixel["y"], pixel["x"], value, mode), bad)
    print(f"{case['name']}: NaN pixels outside scipy's set, summed over the case's inputs, per mode: {outside}")
    assert not bad, (len(bad), bad[:4])


def _map_smooth(ctx, data, weight, sy, sx, want_denom=True):
    import torch

    from maria_amd._lib import ptr

    dev = "cuda:0"
    ny, nx = data.shape
    d_data = torch.as_tensor(data).to(dev)
    d_w = torch.as_tensor(weight).to(dev) if weight is not None else None
    d_out = torch.empty_like(d_data)
    d_den = torch.full_like(d_data, -7.5) if want_denom else None
    d_tmp = torch.empty(2 * ny * nx, dtype=torch.float32, device=dev)
    ctx.call("mrx_map_smooth", ptr(d_data), ptr(d_w), ptr(d_out), ptr(d_den), ptr(d_tmp), ny, nx, float(sy), float(sx))
    return d_out.cpu().numpy(), (d_den.cpu().numpy() if want_denom else None)


def test_map_smooth_with_unhit_pixels(gpu_ctx):
    """A binned map: NaN data under zero weight where no sample fell, and one pixel of infinite weight elsewhere.
    numer = G(data * weight) and denom = G(weight) against oracle.hotpath.map_smooth: the NaN and Inf sets as sets, the
    finite quotients inside (e_n + |out| e_d) / min denom + two float32 roundings of the quotient, e_n and e_d the
    stencil's bound on numerator and denominator."""
    from oracle import hotpath

    rng = np.random.default_rng(21)
    ny, nx = 100, 150
    sy, sx = 2.0, 3.5  # radii 8 and 14
    data = rng.standard_normal((ny, nx)).astype(np.float32)
    weight = (0.5 + rng.random((ny, nx))).astype(np.float32)
    data[50, 40], weight[50, 40] = np.nan, 0.0
    weight[50, 105] = np.inf
    with np.errstate(invalid="ignore"):
        ref, ref_den = hotpath.map_smooth(data, weight, sy, sx)
        ref_num = gc.reference(data * weight, sy, sx)
    ref = ref.astype(np.float32)
    assert np.isnan(ref).any() and not np.isfinite(ref_den).all()
    ys, xs = np.nonzero(~np.isfinite(ref) | ~np.isfinite(ref_den))
    assert min(ys.min(), ny - 1 - ys.max(), xs.min(), nx - 1 - xs.max()) >= gc.NONFINITE_MARGIN
    fin = np.isfinite(ref) & np.isfinite(ref_den)
    for mode in gc.ALL_MODES:
        b = gc.BOUND[mode]
        with _mode(gpu_ctx, mode):
            got, den = _map_smooth(gpu_ctx, data, weight, sy, sx)
        bad = []
        _check_nonfinite(den, ref_den, b, ("denom", mode), bad)
        e_n = b * max(1.0, float(np.abs(ref_num[np.isfinite(ref_num)]).max()))
        e_d = b * max(1.0, float(np.abs(ref_den[np.isfinite(ref_den)]).max()))
        out_max = float(np.abs(ref[fin]).max())
        tol = (e_n + out_max * e_d) / float(ref_den[fin].min()) + 2.0 ** -23 * out_max
        assert ref_den[fin].min() > 0.4
        _check_nonfinite(got, ref, tol / max(1.0, out_max), ("out", mode), bad)
        assert not bad, bad


def test_map_smooth_corners(gpu_ctx):
    """No weight anywhere gives zeros (never 0 / 0); the denominator buffer is optional; a weight of one is no weight."""
    rng = np.random.default_rng(22)
    ny, nx = 70, 130
    data = rng.standard_normal((ny, nx)).astype(np.float32)
    weight = rng.random((ny, nx)).astype(np.float32)
    out, den = _map_smooth(gpu_ctx, data, np.zeros_like(data), 2.0, 3.5)
    assert (out == 0).all() and (den == 0).all()
    a, _ = _map_smooth(gpu_ctx, data, weight, 2.0, 3.5, want_denom=True)
    b, _ = _map_smooth(gpu_ctx, data, weight, 2.0, 3.5, want_denom=False)
    assert np.array_equal(_bits(a), _bits(b))
    # uniform weights: the denominator G(1) is written as exactly 1.0f (scipy's is within 1e-6 of it) ...
    plain, den = _map_smooth(gpu_ctx, data, None, 2.0, 3.5)
    assert (den == np.float32(1.0)).all()
    assert np.abs(gc.reference(np.ones_like(data), 2.0, 3.5) - 1.0).max() <= 1e-6
    # ... which is what the kernels make of a plane of ones in float64 (taps normalised in float64: a sum within a few
    # 1e-16 of 1 rounds to 1.0f), so the weighted form with ones gives the same bits
    with _mode(gpu_ctx, 1):
        ones, den1 = _map_smooth(gpu_ctx, data, np.ones_like(data), 2.0, 3.5)
        plain1, _ = _map_smooth(gpu_ctx, data, None, 2.0, 3.5)
    assert (den1 == np.float32(1.0)).all() and np.array_equal(_bits(ones), _bits(plain1))
