"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle.

Tolerances (north_star: TOD within 1e-5 relative of the CPU reference, fp32):
  * total loading / TOD in pW:  max|d| / max|ref| <= 1e-5     (asserted)
  * coarse pwv (float64 accumulator of float32 terms): <= 2e-6 relative
  * fluctuation-only error (mean removed per detector) is reported and
    bounded by 1e-3: the float32 trig of OCML and of numpy differ by an ulp,
    which moves a line of sight by ~1e-3 m on a 10 km layer.
"""

import numpy as np
import pytest
import scipy.interpolate

from helpers import rel_err, small_problem

pytestmark = pytest.mark.gpu

TOL_TOD = 1e-5


def _device_path(problem, **kw):
    from maria_amd.pipeline import DevicePath

    return DevicePath(problem, device="cuda:0", **kw)


# Fluctuation-only bounds (per-detector mean removed, relative to the largest fluctuation): 2x the largest
# value measured on the GPU in round 3 (printed by the tests; pytest -s).  The loading is a float32 number
# dominated by its mean, so its rounding (a few ulp, ~4e-7 of the value) is ~3e-5 of a 1.4 % fluctuation;
# the TOD adds the spline's extrapolated tail, where knot differences grow ~3.5x.  Measured: coarse loading
# 5.5e-5 ... 8.8e-5 (three shapes, both pointing modes), pixel rule vs literal rule 6.6e-5, TOD 2.4e-4.
# (The float64 pwv -- the turbulent signal before the float32 emission lookup -- agrees to 3e-6 of its own
# fluctuation at full size: tests/test_gpu_fullsize.py.)
FLUCT_TOL_COARSE = 1.8e-4
FLUCT_TOL_TOD = 5e-4


def _fluct_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    fa = a - a.mean(axis=-1, keepdims=True)
    fb = b - b.mean(axis=-1, keepdims=True)
    return np.abs(fa - fb).max() / max(np.abs(fb).max(), 1e-300)


@pytest.mark.parametrize("chain", [0, 1], ids=["direct", "chain"])
@pytest.mark.parametrize("n_det,n_layers,n_bands", [(67, 3, 2), (300, 1, 1), (16, 8, 3)])
def test_sample_matches_oracle(gpu_ctx, n_det, n_layers, n_bands, chain):
    """Both pointing modes of mrx_atm_sample (MRX_OPT_POINTING_CHAIN) against the
    oracle, which restates the reference's float32 chain."""
    from maria_amd import _lib
    from oracle import hotpath

    p = small_problem(n_det=n_det, n_layers=n_layers, n_bands=n_bands)
    path = _device_path(p, ctx=gpu_ctx, keep_pwv=True)
    gpu_ctx.set_option(_lib.OPT_POINTING_CHAIN, chain)
    try:
        path.sample()
    finally:
        gpu_ctx.set_option(_lib.OPT_POINTING_CHAIN, 0)
    assert path.check_flags() == 0
    got_pwv = path.coarse_pwv().cpu().numpy()
    got = path.coarse_loading().cpu().numpy()

    _, inter = hotpath.run_path(p, return_intermediates=True)
    assert rel_err(got_pwv, inter["pwv"]) <= 2e-6
    assert rel_err(got, inter["loading_a"]) <= TOL_TOD
    fe = _fluct_err(got, inter["loading_a"])
    print(f"MEASURED sample fluct {n_det}/{n_layers}/{n_bands}/chain={chain}: {fe:.3e}")
    assert fe <= FLUCT_TOL_COARSE


def test_nonuniform_axes_take_the_array_path(gpu_ctx):
    """A layer whose axis is not float32(g0 + i*dg) (here: a stretched grid, and a
    uniform one given without a usable hint) is searched in the axis array; results
    still match the oracle, which interpolates on the same arrays."""
    from oracle import hotpath

    p = small_problem(n_det=40, n_layers=3, n_bands=1)
    uniform_path = _device_path(p, ctx=gpu_ctx)
    assert uniform_path.plan_info() == (6, True)
    # stretch layer 1's cross-section axis smoothly (still ascending, covers the samples)
    ax = p["layers"][1]["cross_section"]
    mid = 0.5 * (ax[0] + ax[-1])
    p["layers"][1]["cross_section"] = mid + (ax - mid) * (1.0 + 0.3 * ((ax - mid) / (ax[-1] - mid)) ** 2)
    # and perturb one node of layer 2's extrusion axis by less than a step
    ex = p["layers"][2]["extrusion"].copy()
    ex[len(ex) // 2] += 0.4 * (ex[1] - ex[0])
    p["layers"][2]["extrusion"] = ex
    path = _device_path(p, ctx=gpu_ctx, keep_pwv=True)
    assert path.plan_info()[0] == 4
    path.sample()
    assert path.check_flags() == 0
    _, inter = hotpath.run_path(p, return_intermediates=True)
    assert rel_err(path.coarse_pwv().cpu().numpy(), inter["pwv"]) <= 2e-6
    assert rel_err(path.coarse_loading().cpu().numpy(), inter["loading_a"]) <= TOL_TOD


def test_large_band_tables_take_the_global_path(gpu_ctx):
    """Band tables too large for the kernel's 48 KiB LDS stage are read from global
    memory (mrx_atm_plan_info reports it); same results."""
    from maria_amd import synthetic
    from oracle import hotpath

    p = small_problem(n_det=90, n_layers=2, n_bands=3)
    p["tables"] = synthetic.emission_tables(3, n_pwv=80, n_el=90)
    path = _device_path(p, ctx=gpu_ctx, keep_pwv=True)
    assert path.plan_info()[1] is False
    path.sample()
    assert path.check_flags() == 0
    _, inter = hotpath.run_path(p, return_intermediates=True)
    assert rel_err(path.coarse_loading().cpu().numpy(), inter["loading_a"]) <= TOL_TOD


def test_emission_table_out_of_range_gives_nan_like_jax(gpu_ctx):
    """pwv outside the table: jax's interpolator fills NaN (band/band.py:283-286); the
    kernel writes NaN and raises MRX_FLAG_TABLE_OOB, the screens are fine."""
    from maria_amd import _lib

    p = small_problem(n_det=20, n_layers=1, n_bands=1)
    p["pwv0"] = 25.0  # the synthetic table ends at 10 mm
    path = _device_path(p, ctx=gpu_ctx)
    path.clear_flags()
    path.sample()
    flags = path.check_flags()
    assert flags & _lib.FLAG_TABLE_OOB and flags & _lib.FLAG_NAN and not flags & _lib.FLAG_SCREEN_OOB
    assert np.isnan(path.d_loading.cpu().numpy()).all()


def test_pixel_coordinates_agree_with_the_literal_cell_search(gpu_ctx):
    """On verified-uniform axes the kernel takes cell and weight from the position in pixels
    (default: a float64 anchor per step and layer + the lane's float32 offset from it, good to
    ~4e-6 pixel); MRX_OPT_AXIS_LITERAL searches the float32 axis arrays with jax's rule instead.
    The two differ only by the float32 rounding of the reference's own coordinates (~2e-4 pixel
    at 10 km from the grid origin): far inside the parity tolerance, and both match the oracle."""
    from oracle import hotpath

    p = small_problem(n_det=200, n_layers=4, n_bands=2)
    path = _device_path(p, ctx=gpu_ctx, keep_pwv=True)
    assert path.plan_info()[0] == 8
    path.sample()
    a_load, a_pwv = path.d_loading.clone(), path.d_pwv.clone()
    gpu_ctx.set_option(1, 1)
    try:
        path.sample()
    finally:
        gpu_ctx.set_option(1, 0)
    assert path.check_flags() == 0
    b_load, b_pwv = path.d_loading, path.d_pwv
    assert rel_err(a_pwv.cpu().numpy(), b_pwv.cpu().numpy()) <= 2e-7
    assert rel_err(a_load.cpu().numpy(), b_load.cpu().numpy()) <= 1e-6
    fe = _fluct_err(a_load.cpu().numpy().T, b_load.cpu().numpy().T)
    print(f"MEASURED pixel-vs-literal fluct: {fe:.3e}")
    assert fe <= FLUCT_TOL_COARSE
    _, inter = hotpath.run_path(p, return_intermediates=True)
    for pwv in (a_pwv, b_pwv):
        assert rel_err(pwv.T.index_select(0, path._d_inverse).cpu().numpy(), inter["pwv"]) <= 2e-6


def test_full_path_matches_oracle(gpu_ctx):
    from oracle import hotpath

    p = small_problem(gain=True)
    path = _device_path(p, ctx=gpu_ctx)
    tod = path.run().cpu().numpy()
    assert path.check_flags() == 0
    ref = hotpath.run_path(p)
    assert tod.shape == ref.shape and tod.dtype == np.float32
    assert rel_err(tod, ref) <= TOL_TOD
    fe = _fluct_err(tod, ref)
    print(f"MEASURED full-path fluct: {fe:.3e}")
    assert fe <= FLUCT_TOL_TOD


def _spline_upsample(gpu_ctx, form, d_y, D, Ta, ta0, dta, d_t, T, d_scale, d_out, ld):
    """The two forms of the cubic upsample through the C ABI: "fused" = mrx_spline_upsample_fused (the
    solve in the writer's tile prologue, what DevicePath.run launches), "two-call" = mrx_spline_prepare +
    mrx_spline_upsample.  Returns the (y, m) knots of the two-call form (None for the fused one)."""
    import torch

    from maria_amd._lib import ptr

    if form == "fused":
        gpu_ctx.call("mrx_spline_upsample_fused", ptr(d_y), D, Ta, ta0, dta, ptr(d_t), T, ptr(d_scale), None, ptr(d_out), ld)
        return None
    d_ym = torch.empty((Ta, D, 2), dtype=torch.float32, device=d_y.device)
    gpu_ctx.call("mrx_spline_prepare", ptr(d_y), D, Ta, ptr(d_ym))
    gpu_ctx.call("mrx_spline_upsample", ptr(d_ym), D, Ta, ta0, dta, ptr(d_t), T, ptr(d_scale), None, ptr(d_out), ld)
    return d_ym


@pytest.mark.parametrize("form", ["fused", "two-call"])
@pytest.mark.parametrize("Ta", [4, 5, 6, 7, 15, 16, 17, 31, 33, 48, 49, 100, 601])
def test_spline_matches_scipy_all_lengths(gpu_ctx, Ta, form):
    """Both forms of the cubic upsample against scipy's not-a-knot cubic on the same coarse
    samples, including the extrapolated tail (sim/atmosphere.py:72-82) and samples before the
    first knot."""
    import torch

    rng = np.random.default_rng(Ta)
    D = 37
    t0 = 1.7e9
    ta = np.arange(t0, t0 + Ta * 0.1 - 1e-9, 0.1)[:Ta]
    assert len(ta) == Ta
    y = (20 + np.cumsum(rng.standard_normal((D, Ta)), axis=1) * 0.05).astype(np.float32)
    t = np.arange(ta[0] - 0.05, ta[-1] + 0.15, 1 / 47.0)  # not a multiple of 4, both tails
    T = len(t)
    ref = scipy.interpolate.interp1d(ta, y, kind="cubic", bounds_error=False, fill_value="extrapolate", axis=-1)(t)

    dev = "cuda:0"
    d_y = torch.as_tensor(np.ascontiguousarray(y.T)).to(dev)
    d_t = torch.as_tensor(t).to(dev)
    ld = T + 3  # odd pitch: exercises the scalar-store path
    d_out = torch.full((D, ld), -7.0, dtype=torch.float32, device=dev)
    d_ym = _spline_upsample(gpu_ctx, form, d_y, D, Ta, float(ta[0]), float(ta[1] - ta[0]), d_t, T, None, d_out, ld)
    out = d_out.cpu().numpy()
    assert (out[:, T:] == -7.0).all(), "wrote past T"
    # measured 4e-8 ... 9e-8: the float32 rounding of the value itself (round 2's evaluation form: 1e-6)
    assert rel_err(out[:, :T], ref) <= 2e-7
    if d_ym is not None:  # knots are reproduced (interpolation property)
        assert np.array_equal(d_ym.cpu().numpy()[:, :, 0], y.T)


@pytest.mark.parametrize("form", ["fused", "two-call"])
@pytest.mark.parametrize("ratio", [1.0, 2.5, 3.9, 8.0, 17.0, 19.0, 40.0, 400.0])
def test_upsample_ratios(gpu_ctx, ratio, form):
    """Every tile path of the evaluation kernels.  Two-call form: ratios below ~4 take the
    global-load path, the others stage knots through LDS.  Fused form: the 64-knot image (two row
    groups per pass) from ~18 up, the 256-knot image down to ~4, segments of one tile below."""
    import torch

    rng = np.random.default_rng(3)
    D, Ta = 50, 700
    ta = 100.0 + 0.1 * np.arange(Ta)
    y = (5 + rng.standard_normal((D, Ta)).cumsum(axis=1) * 0.01).astype(np.float32)
    t = np.arange(ta[0], ta[-1] + 0.1, 0.1 / ratio)
    T = len(t) - len(t) % 4
    t = t[:T]
    ref = scipy.interpolate.interp1d(ta, y, kind="cubic", bounds_error=False, fill_value="extrapolate", axis=-1)(t)
    dev = "cuda:0"
    d_y = torch.as_tensor(np.ascontiguousarray(y.T)).to(dev)
    d_t = torch.as_tensor(t).to(dev)
    d_out = torch.full((D, T), float("nan"), dtype=torch.float32, device=dev)
    scale = rng.uniform(0.5, 2.0, D).astype(np.float32)
    d_scale = torch.as_tensor(scale).to(dev)
    _spline_upsample(gpu_ctx, form, d_y, D, Ta, float(ta[0]), 0.1, d_t, T, d_scale, d_out, T)
    assert rel_err(d_out.cpu().numpy(), ref * scale[:, None]) <= 2e-7  # measured 9e-8: the value's rounding and the gain's


def test_fused_upsample_equals_the_two_call_form(gpu_ctx):
    """The fused writer against prepare + upsample on white-noise knots (the hardest case for the
    truncated sweeps: second differences as large as the values), 700 rows x 6000 knots x ratio 40, rows
    through a destination permutation: equal to float32 rounding of m."""
    import torch

    from maria_amd._lib import ptr

    rng = np.random.default_rng(11)
    D, Ta, ratio = 700, 6000, 40
    y = rng.standard_normal((Ta, D)).astype(np.float32)
    T = Ta * ratio
    t = 5.0 + np.arange(T) * (0.1 / ratio)
    dev = "cuda:0"
    d_y, d_t = torch.as_tensor(y).to(dev), torch.as_tensor(t).to(dev)
    rows = torch.as_tensor(rng.permutation(D).astype(np.int32)).to(dev)
    a = torch.empty((D, T), dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    d_ym = torch.empty((Ta, D, 2), dtype=torch.float32, device=dev)
    gpu_ctx.call("mrx_spline_prepare", ptr(d_y), D, Ta, ptr(d_ym))
    gpu_ctx.call("mrx_spline_upsample", ptr(d_ym), D, Ta, 5.0, 0.1, ptr(d_t), T, None, ptr(rows), ptr(a), T)
    gpu_ctx.call("mrx_spline_upsample_fused", ptr(d_y), D, Ta, 5.0, 0.1, ptr(d_t), T, None, ptr(rows), ptr(b), T)
    assert float((a - b).abs().max()) <= 2e-7 * float(a.abs().max())


def test_linear_upsample(gpu_ctx):
    import torch

    from maria_amd._lib import ptr
    from oracle import hotpath

    rng = np.random.default_rng(5)
    D, Ta = 33, 90
    ta = 0.1 * np.arange(Ta)
    pwv = 1 + 0.01 * rng.standard_normal((D, Ta))
    t = np.arange(0, ta[-1] + 0.09, 0.02)
    ref = hotpath.upsample_linear(ta, pwv, t)
    dev = "cuda:0"
    d_p = torch.as_tensor(np.ascontiguousarray(pwv.T)).to(dev)
    d_t = torch.as_tensor(t).to(dev)
    d_out = torch.empty((D, len(t)), dtype=torch.float32, device=dev)
    gpu_ctx.call("mrx_linear_upsample", ptr(d_p), D, Ta, 0.0, 0.1, ptr(d_t), len(t), ptr(d_out), len(t))
    assert rel_err(d_out.cpu().numpy(), ref) <= 2e-7


_LINEAR_GRIDS = [(0.0, 0.1), (1.7e9, 0.1), (1.7e9 + 0.3, 0.04), (1.7e9, 1.0 / 3.0)]


def _linear_times(rng, ta, dta, T):
    """T unsorted times: the two extremes (3 dta outside the knots), every knot exactly, uniform draws between the
    extremes -- as many of them, in that order of preference, as T holds."""
    lo, hi = ta[0] - 3.0 * dta, ta[-1] + 3.0 * dta
    must = np.concatenate([[lo, hi], ta])[:T]
    t = np.concatenate([must, rng.uniform(lo, hi, T - len(must))])
    return t[rng.permutation(T)]


def _linear_bound(ta0, dta, pwv, t, ref):
    """Per sample: 2^-24 |ref| + 8 2^-53 |ref| + 4 2^-53 (max|t| / dta) max_j |y_j+1 - y_j| max(1, |u|)."""
    Ta = pwv.shape[1]
    step = np.abs(np.diff(pwv, axis=1)).max(axis=1)[:, None]
    jj = np.clip(np.floor((t - ta0) / dta), 0, Ta - 2)
    u = np.abs((t - (ta0 + jj * dta)) / dta)[None, :]
    return (2.0 ** -24 + 8 * 2.0 ** -53) * np.abs(ref) + 4 * 2.0 ** -53 * (np.abs(t).max() / dta) * step * np.maximum(1.0, u)


@pytest.mark.parametrize("ta0,dta", _LINEAR_GRIDS)
def test_linear_upsample_layouts_and_epoch_times(gpu_ctx, ta0, dta):
    """mrx_linear_upsample against float64 interp1d with extrapolation (oracle.hotpath.upsample_linear): detector and
    sample counts around the tile (16 rows) and the block (256 samples), two and ninety knots, times at the epoch,
    unsorted, on the knots and up to 3 steps outside them; ld_out = T + 3 with a sentinel.  Per sample
        |out - ref| <= 2^-24 |ref| + 8 2^-53 |ref| + 4 2^-53 (max|t| / dta) max_j |y_j+1 - y_j| max(1, |u|):
    the float32 store, and the float64 roundings of t - ta0, * (1 / dta) and ta0 + j dta, which an epoch-sized t
    amplifies by |t| / dta."""
    import torch

    from maria_amd._lib import ptr
    from oracle import hotpath

    rng = np.random.default_rng(17)
    dev = "cuda:0"
    worst = 0.0
    for Ta in (2, 90):
        ta = ta0 + np.arange(Ta) * dta
        for D in (1, 16, 17, 33):
            pwv = 1 + 0.01 * rng.standard_normal((D, Ta))
            d_p = torch.as_tensor(np.ascontiguousarray(pwv.T)).to(dev)
            for T in (1, 255, 256, 257, 1000):
                t = _linear_times(rng, ta, dta, T)
                ref = hotpath.upsample_linear(ta, pwv, t)
                ld = T + 3
                d_t = torch.as_tensor(t).to(dev)
                d_out = torch.full((D, ld), -9.0, dtype=torch.float32, device=dev)
                gpu_ctx.call("mrx_linear_upsample", ptr(d_p), D, Ta, float(ta0), float(dta), ptr(d_t), T, ptr(d_out), ld)
                got = d_out.cpu().numpy()
                assert (got[:, T:] == -9.0).all()
                bound = _linear_bound(ta0, dta, pwv, t, ref)
                ratio = float((np.abs(got[:, :T].astype(np.float64) - ref) / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (Ta, D, T, ratio)
    print(f"linear upsample, ta0 = {ta0!r}, dta = {dta!r}: worst |out - ref| / bound = {worst:.3f}")


def test_linear_upsample_nan_time_stays_in_its_sample(gpu_ctx):
    import torch

    from maria_amd._lib import ptr
    from oracle import hotpath

    rng = np.random.default_rng(18)
    D, Ta, T = 17, 90, 257
    ta = 1.7e9 + np.arange(Ta) * 0.1
    pwv = 1 + 0.01 * rng.standard_normal((D, Ta))
    t = _linear_times(rng, ta, 0.1, T)
    t[100] = np.nan
    d_p, d_t = torch.as_tensor(np.ascontiguousarray(pwv.T)).to("cuda:0"), torch.as_tensor(t).to("cuda:0")
    d_out = torch.full((D, T), -9.0, dtype=torch.float32, device="cuda:0")
    gpu_ctx.call("mrx_linear_upsample", ptr(d_p), D, Ta, 1.7e9, 0.1, ptr(d_t), T, ptr(d_out), T)
    got = d_out.cpu().numpy()
    bad = np.zeros((D, T), bool)
    bad[:, 100] = True
    assert np.array_equal(np.isnan(got), bad) and np.isfinite(got[~bad]).all()
    ok = np.arange(T) != 100
    ref = hotpath.upsample_linear(ta, pwv, t[ok])
    assert (np.abs(got[:, ok].astype(np.float64) - ref) <= _linear_bound(1.7e9, 0.1, pwv, t[ok], ref)).all()


def test_out_of_screen_raises_like_reference(gpu_ctx):
    """atmosphere/atmosphere.py:368-369: a sample outside a layer's grid is NaN and
    the reference raises RuntimeError; the kernel flags it and the host raises."""
    p = small_problem(n_layers=2)
    p["layers"][1]["extrusion"] = p["layers"][1]["extrusion"] + 400.0  # shift the grid away
    path = _device_path(p, ctx=gpu_ctx)
    path.clear_flags()
    path.sample()
    with pytest.raises(RuntimeError, match="introduced nans"):
        path.check_flags()
    assert np.isnan(path.d_loading.cpu().numpy()).any()


@pytest.mark.parametrize("literal", [0, 1], ids=["pixel", "literal"])
def test_degenerate_pointing_is_flagged_not_faulted(gpu_ctx, literal):
    """Lines of sight at or below the horizon (the reference refuses such observations up front,
    sim/observation.py:61-71; the C ABI has no such guard) and NaN pointing: the ground projection is
    infinite or NaN, every cell index is clamped into its screen, the samples come out NaN with
    MRX_FLAG_SCREEN_OOB -- and detectors with a sane pointing in the same launch keep their values."""
    from maria_amd import _lib

    p = small_problem(n_det=70, n_layers=3, n_bands=1)
    good = _device_path(p, ctx=gpu_ctx)
    gpu_ctx.set_option(_lib.OPT_AXIS_LITERAL, literal)
    try:
        good.sample()
    finally:
        gpu_ctx.set_option(_lib.OPT_AXIS_LITERAL, 0)
    want = good.coarse_loading().cpu().numpy()
    assert good.check_flags() == 0
    q = dict(p)
    off = np.array(p["offsets"], float)
    off[3] = [0.0, -np.radians(70.0)]   # 70 degrees below the boresight: under the horizon
    off[11] = [np.nan, 0.0]
    q["offsets"] = off
    path = _device_path(q, ctx=gpu_ctx)
    path.clear_flags()
    gpu_ctx.set_option(_lib.OPT_AXIS_LITERAL, literal)
    try:
        path.sample()
    finally:
        gpu_ctx.set_option(_lib.OPT_AXIS_LITERAL, 0)
    with pytest.raises(RuntimeError, match="introduced nans"):
        path.check_flags()
    got = path.coarse_loading().cpu().numpy()
    assert np.isnan(got[11]).all() and np.isnan(got[3]).any()
    keep = np.setdiff1d(np.arange(70), [3, 11])
    assert np.array_equal(got[keep], want[keep])


def test_empty_shard_and_errors(gpu_ctx):
    import torch

    from maria_amd import MrxError
    from maria_amd._lib import ptr

    p = small_problem()
    path = _device_path(p, ctx=gpu_ctx, det_slice=slice(5, 5))
    assert path.D == 0
    out = path.run()
    assert tuple(out.shape) == (0, path.T)
    # fewer than 4 coarse samples: scipy's cubic raises, so does the library
    d = torch.zeros((3, 4), dtype=torch.float32, device="cuda:0")
    ym = torch.zeros((3, 4, 2), dtype=torch.float32, device="cuda:0")
    with pytest.raises(MrxError, match="UNSUPPORTED"):
        gpu_ctx.call("mrx_spline_prepare", ptr(d), 4, 3, ptr(ym))
    with pytest.raises(MrxError, match="INVALID"):
        gpu_ctx.call("mrx_spline_prepare", None, 4, 8, ptr(ym))
    t = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    o = torch.zeros((4, 8), dtype=torch.float32, device="cuda:0")
    with pytest.raises(MrxError, match="UNSUPPORTED"):
        gpu_ctx.call("mrx_spline_upsample_fused", ptr(d), 4, 3, 0.0, 0.1, ptr(t), 8, None, None, ptr(o), 8)
    with pytest.raises(MrxError, match="INVALID"):
        gpu_ctx.call("mrx_spline_upsample_fused", ptr(d), 4, 8, 0.0, 0.1, ptr(t), 8, None, None, ptr(o), 4)  # ld < T


def test_shard_rows_are_bit_identical(gpu_ctx):
    """Detector sharding: a shard computes exactly the rows the whole
    array would."""
    p = small_problem(n_det=301, n_bands=3, gain=True)
    whole = _device_path(p, ctx=gpu_ctx).run().cpu().numpy()
    for sl in [slice(0, 100), slice(100, 117), slice(117, 301)]:
        part = _device_path(p, ctx=gpu_ctx, det_slice=sl).run().cpu().numpy()
        assert np.array_equal(part, whole[sl])


def test_allgather_through_the_c_abi_single_rank(gpu_ctx):
    """mrx_comm_create + mrx_allgather_tod (RCCL loaded by libmrx) with a communicator of one
    rank: in place it leaves the buffer as the writer filled it, out of place it copies the shard
    into slot 0.  The multi-rank path is the same call with world > 1 (bench.py --gpus N)."""
    import torch

    from maria_amd.dist import TodGather

    n_det, T = 37, 1000
    g = TodGather(gpu_ctx, n_det, world=1, rank=0)
    assert (g.lo, g.hi, g.rows_per_rank) == (0, n_det, n_det)
    full = g.full_buffer(T, "cuda:0")
    rows = g.my_rows(full)
    rows.copy_(torch.arange(n_det * T, dtype=torch.float32, device="cuda:0").reshape(n_det, T))
    want = rows.clone()
    out = g.gather(full)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    shard = torch.rand((n_det, T), dtype=torch.float32, device="cuda:0")
    out = g.gather(full, shard=shard)
    torch.cuda.synchronize()
    assert torch.equal(out, shard)
    assert g.bytes_received(T) == 0
    # the direct form (grouped sends / receives: none with one rank) and the layer exchange (one
    # grouped broadcast per layer from its owner, here rank 0 itself) on the same communicator
    shard2 = torch.rand((n_det, T), dtype=torch.float32, device="cuda:0")
    out = g.gather(full, shard=shard2, algo="p2p")
    torch.cuda.synchronize()
    assert torch.equal(out, shard2)
    screens = [torch.rand((64, 48 + l), dtype=torch.float32, device="cuda:0") for l in range(3)]
    keep = [t.clone() for t in screens]
    g.exchange_screens(screens)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(screens, keep))
    g.close()


def test_cubic_emission_lookup_matches_scipy(gpu_ctx):
    """interpolation_method="cubic" (band/band.py:288-300): linear in T, then scipy's
    RegularGridInterpolator(method="cubic") on (pwv, el) in float64 -- in the kernel as one
    bicubic per table cell expanded from scipy's own spline object."""
    from maria_amd.pipeline import DevicePath
    from oracle import hotpath

    p = small_problem(n_det=83, n_bands=2, n_layers=3)
    p["interpolation_method"] = "cubic"
    path = DevicePath(p, device="cuda:0", ctx=gpu_ctx, keep_pwv=True)
    tod = path.run().cpu().numpy()
    assert path.check_flags() == 0
    ref, mid = hotpath.run_path(p, return_intermediates=True)
    got_a = path.coarse_loading().cpu().numpy()
    assert rel_err(got_a, mid["loading_a"]) <= 2e-6
    assert rel_err(tod, ref) <= 1e-5
    # not the linear lookup: the two methods differ by far more than the tolerance
    p_lin = dict(p, interpolation_method="linear")
    lin = DevicePath(p_lin, device="cuda:0", ctx=gpu_ctx).run().cpu().numpy()
    assert rel_err(lin, ref) > 1e-4
    # scipy raises ValueError outside the grid (bounds_error=True), jax's linear lookup gives NaN
    hot = dict(p, pwv0=11.5)  # beyond the table's 10 mm
    bad = DevicePath(hot, device="cuda:0", ctx=gpu_ctx)
    bad.run()
    with pytest.raises(ValueError, match="out of bounds"):
        bad.check_flags()
    with pytest.raises(ValueError):
        DevicePath(dict(p, T0=100.0), device="cuda:0", ctx=gpu_ctx)  # interp1d refuses a T0 off the axis


@pytest.mark.gpu
def test_side_streams_are_chosen_off_the_callers_hardware_queue(gpu_ctx):
    """HIP spreads streams round-robin over four hardware queues: one new stream in four shares the caller's
    and would run the pipelined step's sampler behind the writer instead of beside it (2.9 instead of 2.1 ms at
    the headline size).  mrx_streams_concurrent sees it (two spin kernels, timed); DevicePath takes a stream
    that passes, whichever stream is current."""
    import torch

    from maria_amd import synthetic
    from maria_amd.pipeline import DevicePath

    main = torch.cuda.current_stream()
    gpu_ctx.set_stream(main)
    assert not gpu_ctx.streams_concurrent(main)  # a stream is not beside itself
    verdicts = [gpu_ctx.streams_concurrent(torch.cuda.Stream()) for _ in range(8)]
    assert any(verdicts)  # (on the default four queues: six of eight)
    p = synthetic.make_problem(n_det=64, n_bands=1, fov_deg=0.5, fs=50.0, duration=20.0, n_layers=2, side=128)
    path = DevicePath(p, device="cuda:0", ctx=gpu_ctx)
    for cur in (main, torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(cur):
            side = path._side_stream(cur)
            gpu_ctx.set_stream(cur)
            assert gpu_ctx.streams_concurrent(side)
    gpu_ctx.set_stream(main)


def test_overlapping_runs_are_bit_identical_to_separate_ones(gpu_ctx):
    """DevicePath.enable_lookahead: the screens of the next observation are generated on their own stream into a
    second buffer set while this one's samplers and writers run, and the samplers start as soon as their screens
    and coarse buffers are free.  Five observations with five different seeds, queued back to back without a
    synchronisation in between, equal the same five made one by one on one stream, bit for bit."""
    import torch

    p = small_problem(n_det=700, n_layers=3, n_bands=1, duration=30.0)
    fast = _device_path(p)
    assert fast.enable_lookahead()
    outs = [torch.empty((fast.D, fast.T), dtype=torch.float32, device="cuda:0") for _ in range(5)]
    for k, out in enumerate(outs):
        p["seed"] = 1000 + 17 * k
        fast.generate_screens()
        fast.run(out=out, blocks=3)
    torch.cuda.synchronize()
    assert fast.check_flags() == 0
    plain = _device_path(p)
    for k, out in enumerate(outs):
        p["seed"] = 1000 + 17 * k
        plain.generate_screens()
        ref = plain.run(blocks=1)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), k
    assert not torch.equal(outs[0], outs[1])


def test_screen_form_does_not_depend_on_the_shard(gpu_ctx):
    """How a screen is generated (the beam as a stencil or folded into the spectrum, whose rim pixels differ) is decided
    from the margins of the WHOLE focal plane: a shard of inner detectors keeps farther from the edges than the array
    does, and must still make -- and sample -- the screens every other shard makes."""
    import torch

    from maria_amd import synthetic
    from maria_amd.pipeline import DevicePath

    p = synthetic.config_problem("atlast_10k", n_det=1024, duration=30.0)
    off = np.asarray(p["offsets"], float)
    inner = slice(0, 64)  # hex_pack orders ring by ring: the first detectors are the central ones
    assert np.hypot(*off[inner].T).max() < 0.5 * np.hypot(*off.T).max()
    whole = DevicePath(p, device="cuda:0", ctx=gpu_ctx)
    part = DevicePath(p, device="cuda:0", ctx=gpu_ctx, det_slice=inner)
    assert part.sampled_margins_px() == whole.sampled_margins_px()
    sw = [s.clone() for s in whole.generate_screens()]
    sp = part.generate_screens()
    assert part._beam_in_spectrum == whole._beam_in_spectrum
    for a, b in zip(sw, sp):
        assert torch.equal(a, b)
    assert torch.equal(part.run(), whole.run()[inner])
