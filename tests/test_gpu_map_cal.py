"""GPU tests of the map sampler's per-sample calibration (mrx_map_sample with calibration tables) where its interval form
(csrc/mrx_map_sample.hip: one parabola record per row and coarse step of a tile) meets its edges: a tile whose end halo sits
on a coarse-step boundary, the halos at the run's two ends, and a tile that meets more coarse steps than the form's
table holds.  Every sample is compared with the oracle (oracle/mapsample.py) and with the kernel's own per-sample form."""

import math

import numpy as np
import pytest

from test_gpu_map import _blob_map, _centre, _rounding_bound

pytestmark = pytest.mark.gpu

_D = 37  # the last 16-row group ragged


def _interval_hits(t, ta0, dta, Ta):
    """The full tiles whose end halo (one sample after the tile's last; the run's last sample's successor when the
    index is clamped) picks record n_int of the interval form, one past the n_int records the tile builds: a numpy
    restatement of step_of, v0, dvt, lim and the halo's choice in mrx_map_sample.hip (float64 steps, float32 v through an
    fma) as they stood before the choice was clamped.  It shows that a case exercises the edge; it is not the reference."""
    t = np.asarray(t, np.float64)
    T, inv_dta, f32 = len(t), 1.0 / dta, np.float32

    def step_of(s):
        tt = t[min(max(s, 0), T - 1)]
        jj = min(max(int(math.floor(min(max((tt - ta0) * inv_dta, -1.0), 2.0e9))), 0), Ta - 2)
        return jj, (tt - (ta0 + jj * dta)) * inv_dta

    hits = []
    for s_tile in range(0, T - 1024 + 1, 1024):
        j_lo = step_of(s_tile - 1)[0]
        n_int = step_of(s_tile + 1024)[0] - j_lo + 1
        if n_int > 64 or n_int * 8 > 1024:
            continue
        sb = s_tile + 1020  # the last thread's first sample
        jb, u_0 = step_of(sb)
        j3, u_3 = step_of(sb + 3)
        v0 = f32(u_0)
        dvt = f32(((j3 - jb) + u_3 - u_0) * (1.0 / 3))
        lim = 3.0e38 if jb >= Ta - 2 else 1.0
        v = f32(4.0 * np.float64(dvt) + np.float64(v0))  # fmaf(4, dvt, v0): 4 dvt is exact
        if v >= lim and jb - j_lo + 1 >= n_int:
            hits.append(s_tile // 1024)
    return hits


def _frontend_grid(t, dta):
    """The coarse grid as the front end builds it: arange over the samples' span, the step from the grid's whole span."""
    ta = np.arange(t.min(), t.max(), dta)
    return ta, ta[0], float((ta[-1] - ta[0]) / (len(ta) - 1))


def _case(name):
    """(t, ta, ta0, dta) of a named case: ``start/rate/step`` on the front end's grid, ``.../nominal`` with the nominal step
    (what a caller of mmap.sample_map passes), ``past_end``: T a multiple of 1024, a caller's grid past t[-1] and a step
    boundary between t[T-1] and one sample later."""
    if name == "past_end":
        fs, T = 400.0, 4096
        t = 12.5 + np.arange(T) / fs
        ta0, dta = 12.439, 0.1  # a boundary at 12.439 + 103 * 0.1 = 22.739, between t[T-1] = 22.7375 and 22.74
        ta = ta0 + np.arange(int((t[-1] - ta0) / dta) + 4) * dta
        return t, ta, ta0, dta
    start, fs, step, *grid = name.split("/")
    t = float(start) + np.arange(10 * 1024 + 300) / float(fs)  # ten whole tiles and a ragged one
    ta, ta0, dta = _frontend_grid(t, float(step))
    if grid:
        dta = float(step)
    return t, ta, ta0, dta


_HITS = ["1.7/400/0.1", "33.3/400/0.1", "1.7/200/0.1", "100.3/400/0.2", "5.0/400/0.2", "1.7e9/400/0.1/nominal",
         "7.3/200/0.1/nominal", "past_end"]
_CONTROLS = ["0.0/400/0.1", "12.5/400/0.1", "1.7e9/400/0.1", "12.5/1000/0.1", "12.5/400/0.5"]

# The interval form against the per-sample form, max |difference| / the row's largest value, measured on an MI355X over
# every case and channel count here: 3.2e-6 to 5.7e-6 at 0.1 and 0.2 s steps, 1.1e-5 at 0.5 s (the parabola over a longer
# step) -- not the 1e-7 the kernel's comment gives for a missed table kink alone.  The bound: 2.3 times the largest.
# The record past the tile's last (before the clamp) put 0.2 to 3e10 of the row's value into the tile's last sample.
_SAME_FORM_BOUND = 2.5e-5


def _sample(ctx, name, C, steps_per_tile=None, seed=0, off_tables=None):
    """The case's TOD through mrx_map_sample with calibration tables, and what the oracle needs to restate it.
    ``off_tables``: a (row, knot) of the coarse pwv put beyond the tables' pwv axis."""
    from maria_amd import map as mmap
    from maria_amd import synthetic

    rng = np.random.default_rng(seed)
    t, ta, ta0, dta = _case(name)
    az, el = synthetic.daisy_scan(t)
    az, el = az.astype(np.float32), el.astype(np.float32)
    off = synthetic.hex_pack(_D, np.radians(0.4))
    centre = _centre(az, el, None)
    eta, xi = np.linspace(0.02, -0.02, 9), np.linspace(-0.02, 0.02, 9)
    X, Y = np.meshgrid(xi, eta)
    # a smooth field of 1 to 1.5 K_RJ (so that the sample's place costs little and the factor shows)
    values = np.stack([(1.0 + (0.5 - 0.1 * c) * np.exp(-((X - 0.004 * c) ** 2 + Y ** 2) / (2 * 0.015 ** 2)))[None] for c in range(C)])
    values = values.astype(np.float32)
    w = np.ones((_D, 1)) * 0.5
    axis_pwv, axis_el = np.linspace(0.0, 6.0, 13), np.radians(np.linspace(20.0, 90.0, 15))
    tabs = np.stack([(1.5e10 + 4e9 * c) * np.exp(-(0.05 + 0.03 * c + 0.04 * axis_pwv[:, None]) / np.sin(axis_el)[None, :])
                     for c in range(C)]).astype(np.float32)
    coarse = 1.2 + 0.3 * np.cumsum(rng.normal(0, 0.05, (_D, len(ta))), axis=1)  # a random walk per detector
    if off_tables is not None:
        coarse[off_tables] = 7.5
    got = mmap.sample_map(ctx, values, eta, xi, centre, az, el, off, w, cal_tables=tabs, cal_axis_pwv=axis_pwv, cal_axis_el=axis_el,
                          coarse_pwv=coarse.T, ta0=ta0, dta=dta, t=t, steps_per_tile=steps_per_tile).cpu().numpy()
    return got, dict(t=t, ta=ta, ta0=ta0, dta=dta, az=az, el=el, off=off, centre=centre, eta=eta, xi=xi, values=values, w=w,
                     tabs=tabs, axis_pwv=axis_pwv, axis_el=axis_el, coarse=coarse)


def _oracle(k):
    from oracle import hotpath, mapsample

    az_d, el_d = hotpath.broadcast(k["off"], k["az"], k["el"])
    # (the oracle's temperature axis: the tables constant in T, so that collapsing it is exact)
    axis_T = np.array([250.0, 290.0])
    tabs3 = [np.stack([tab, tab]) for tab in k["tabs"]]
    ta = k["ta0"] + np.arange(len(k["ta"])) * k["dta"]  # the coarse times the kernel uses
    return mapsample.sample_maps(az_d, el_d, k["t"], ta, k["coarse"], k["eta"], k["xi"], k["centre"], k["values"], k["w"],
                                 cal_tables=tabs3, cal_axes=(axis_T, k["axis_pwv"], k["axis_el"]), base_temperature=273.0)


def _measure(ctx, name, C):
    """(default call, steps_per_tile = 1 call, oracle, the case's data) of one case."""
    got, k = _sample(ctx, name, C)
    per_sample, _ = _sample(ctx, name, C, steps_per_tile=1)
    return got, per_sample, _oracle(k), k


@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("name", _HITS + _CONTROLS)
def test_interval_calibration_on_unaligned_coarse_grids(gpu_ctx, name, C):
    """Coarse grids that do not line up with the samples: where float64 puts a tile's end halo at u = 1 - 1e-14 of a step
    and float32 rounds its place to 1.0, the interval form must not read the record after the tile's last (nothing wrote
    it); at the run's two ends the halo is the end sample itself (scipy's 'reflect').  Every sample against (a) the
    oracle, within test_map_sampling_with_atmospheric_transmission's bound, and (b) the kernel's per-sample form (the
    same call with steps_per_tile = 1, which no tile's interval table fits), within 2.5e-5 of the row's largest value --
    measured up to 5.7e-6 at 0.1-0.2 s steps and 1.1e-5 at 0.5 s on an MI355X, while the unwritten record put 0.2 or more
    of the row's value into the tile's last sample."""
    from oracle import mapsample

    got, per_sample, ref, k = _measure(gpu_ctx, name, C)
    hits = _interval_hits(k["t"], k["ta0"], k["dta"], len(k["ta"]))
    if name in _HITS:
        assert hits, "the case is what it says: some tile's halo sits on a step boundary"
    else:
        assert not hits, hits
    if name == "past_end":
        assert len(k["t"]) % 1024 == 0 and hits == [len(k["t"]) // 1024 - 1] and k["ta"][-1] > k["t"][-1]
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    assert not np.array_equal(got, per_sample), "the interval form ran"
    row = np.abs(per_sample).max(axis=1, keepdims=True)
    bound = _rounding_bound(k["values"], k["eta"], k["xi"], 0.5, 1e12 * mapsample.K_B * sum(tab.max() for tab in k["tabs"]))
    bound_a = bound + 2e-6 * np.abs(ref).max()
    assert bound <= 3e-5 * np.abs(ref).max()
    for tile in hits:  # the tile's first and last column: a wrong record shows in the last
        for s in (tile * 1024, tile * 1024 + 1023):
            e_b = float((np.abs(got[:, s] - per_sample[:, s]) / row[:, 0]).max())
            assert e_b <= _SAME_FORM_BOUND, (tile, s, e_b)
            assert np.abs(got[:, s] - ref[:, s]).max() <= bound_a, (tile, s)
    e_b = float((np.abs(got - per_sample) / row).max())
    assert e_b <= _SAME_FORM_BOUND, (e_b, np.unravel_index(np.argmax(np.abs(got - per_sample) / row), got.shape))
    assert np.abs(got - ref).max() <= bound_a, (float(np.abs(got - ref).max() / np.abs(ref).max()))
    assert np.abs(per_sample - ref).max() <= bound_a


def test_a_row_with_a_knot_off_the_tables_takes_the_per_sample_form(gpu_ctx):
    """One coarse pwv sample of one row lies beyond the tables (NaN: jax's fill).  In the tiles that meet that knot the
    row takes the per-sample form -- its values there are the per-sample call's (steps_per_tile = 1) bit for bit, NaN for
    NaN -- while the tile's other rows stay on the interval form (they differ from the per-sample call's in some bit).
    The NaNs stand where the oracle has them; every other sample within the neighbouring test's bounds."""
    from oracle import mapsample

    name, C, row = "12.5/400/0.1", 2, 21
    t, ta, ta0, dta = _case(name)
    knot = int(round((t[3 * 1024 + 500] - ta0) / dta))  # in the middle of the fourth tile
    got, k = _sample(gpu_ctx, name, C, off_tables=(row, knot))
    per_sample, _ = _sample(gpu_ctx, name, C, steps_per_tile=1, off_tables=(row, knot))
    ref = _oracle(k)
    nan = np.isnan(ref)
    assert nan[row].any() and not np.delete(nan, row, axis=0).any() and not nan[row, : 3 * 1024].any() and not nan[row, 4 * 1024 :].any()
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(per_sample), nan)
    tile = slice(3 * 1024, 4 * 1024)
    assert np.array_equal(got[row, tile], per_sample[row, tile], equal_nan=True), "the row took the per-sample form"
    others = np.delete(np.arange(_D), row)
    assert all(not np.array_equal(got[d, tile], per_sample[d, tile]) for d in others), "the tile's other rows: the interval form"
    assert not np.array_equal(got[row, :1024], per_sample[row, :1024]), "the row in a tile without the knot: the interval form"
    ok = ~nan
    rowmax = np.abs(np.where(ok, per_sample, 0.0)).max(axis=1, keepdims=True)
    bound = _rounding_bound(k["values"], k["eta"], k["xi"], 0.5, 1e12 * mapsample.K_B * sum(tab.max() for tab in k["tabs"]))
    bound_a = bound + 2e-6 * np.abs(ref[ok]).max()
    e_b = float((np.abs(got - per_sample) / rowmax)[ok].max())
    assert e_b <= _SAME_FORM_BOUND, e_b
    assert np.abs(got - ref)[ok].max() <= bound_a and np.abs(per_sample - ref)[ok].max() <= bound_a


def test_more_channels_than_the_interval_table_holds_take_the_per_sample_form(gpu_ctx):
    """Five channels with calibration tables under the composed pointing: the interval table is built for four, so the
    launcher reserves none and every row takes the per-sample form -- the default call equals the steps_per_tile = 1 call
    (which no table fits either) in every bit -- and the field is the oracle's within the neighbouring test's bound."""
    from oracle import mapsample

    got, per_sample, ref, k = _measure(gpu_ctx, "12.5/400/0.1", 5)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    assert np.array_equal(got, per_sample), "no interval table: the per-sample form ran"
    bound = _rounding_bound(k["values"], k["eta"], k["xi"], 0.5, 1e12 * mapsample.K_B * sum(tab.max() for tab in k["tabs"]))
    assert bound <= 3e-5 * np.abs(ref).max()
    assert np.abs(got - ref).max() <= bound + 2e-6 * np.abs(ref).max(), float(np.abs(got - ref).max() / np.abs(ref).max())


def test_krj_sampling_with_more_steps_a_tile_than_the_interval_table(gpu_ctx):
    """50 Hz and 0.1 s coarse steps: a tile meets 207 steps, more than the interval form's 64, so no tile takes it and the
    launcher reserves no table for it.  Four channels and a 200-node K_RJ elevation axis in four bands then fit in the
    60 KiB of mrx_map_sample_krj (with the dead table of 4 x 16 x 193 floats they did not); the call equals mrx_map_sample
    followed by mrx_tod_to_krj bit for bit, NaN for NaN."""
    import torch

    from maria_amd import map as mmap
    from maria_amd import synthetic
    from maria_amd._lib import ptr

    rng = np.random.default_rng(50)
    D, T, C, fs, dta = _D, 3001, 4, 50.0, 0.1
    t = 1.7e9 + np.arange(T) / fs
    az, el = synthetic.daisy_scan(t)
    az, el = az.astype(np.float32), el.astype(np.float32)
    off = synthetic.hex_pack(D, np.radians(0.4))
    centre = _centre(az, el, None)
    eta, xi = np.linspace(0.02, -0.02, 9), np.linspace(-0.02, 0.02, 9)

    values = _blob_map(C, 1, 9, 9, eta, xi, rng)
    w = np.ones((D, 1)) * 0.5
    axis_pwv, axis_el_s = np.linspace(0.0, 6.0, 13), np.radians(np.linspace(20.0, 90.0, 15))
    tabs = np.stack([(1.5e10 + 4e9 * c) * np.exp(-(0.05 + 0.03 * c + 0.04 * axis_pwv[:, None]) / np.sin(axis_el_s)[None, :]) for c in range(C)])
    ta, ta0, dta = _frontend_grid(t, dta)
    coarse = 1.2 + 0.3 * np.cumsum(rng.normal(0, 0.05, (D, len(ta))), axis=1)
    steps = mmap.steps_per_tile(t, dta)
    kw = dict(cal_tables=tabs.astype(np.float32), cal_axis_pwv=axis_pwv, cal_axis_el=axis_el_s, coarse_pwv=coarse.T, ta0=ta0, dta=dta, t=t)
    n_el, n_bands = 200, 4
    # the premise: the sampler's tables and the K_RJ cells fit in 60 KiB, and would not beside a dead interval table
    cal_bytes = 4 * (len(axis_pwv) + len(axis_el_s) + C * len(axis_pwv) * len(axis_el_s))
    krj_bytes = 16 * (n_el - 1) * n_bands
    dead = 4 * C * 16 * (3 * 64 + 1)
    assert steps > 64 and cal_bytes + krj_bytes <= 60 * 1024 < (cal_bytes + dead + 15) // 16 * 16 + krj_bytes
    dev = "cuda:0"
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    axis = np.radians(np.linspace(20.0, 90.0, n_el))
    den = np.stack([(2.0e-2 + 5e-3 * b) * np.exp(-(0.04 + 0.02 * b) / np.sin(axis)) for b in range(n_bands)])
    krj = dict(bore_el=f32(el), dx=f32(off[:, 0]), dy=f32(off[:, 1]), band=torch.as_tensor(rng.integers(0, n_bands, D).astype(np.int32)).to(dev),
               axis=f32(axis), values=f32(den))
    scale = f32(rng.uniform(0.9, 1.1, D))
    ref = mmap.sample_map(gpu_ctx, values, eta, xi, centre, az, el, off, w, **kw)
    ref *= scale[:, None]
    gpu_ctx.call("mrx_tod_to_krj", ptr(ref), ref.stride(0), D, T, None, None, ptr(krj["bore_el"]), ptr(krj["dx"]), ptr(krj["dy"]),
                 ptr(krj["band"]), ptr(krj["axis"]), ptr(krj["values"]), n_el, n_bands)
    got = mmap.sample_map(gpu_ctx, values, eta, xi, centre, az, el, off, w, krj=krj, scale=scale, **kw)
    nan_ref, nan_got = torch.isnan(ref), torch.isnan(got)
    assert torch.equal(nan_ref, nan_got)
    assert torch.equal(torch.where(nan_ref, torch.zeros_like(ref), ref), torch.where(nan_got, torch.zeros_like(got), got)), \
        float((got - ref).abs().nan_to_num().max())
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
