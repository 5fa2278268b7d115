"""The map pixel of every sample against an exact pointing: mrx_map_project, mrx_map_sample, mrx_bin_map and
mrx_bin_map_bucketed on fine grids whose zero is on no node, with samples beyond every edge and, in one case, offsets past
0.1 rad -- each sample held to the set of pixels the reference accepts for it (tests/pointing_ref.py); no share of the
samples may differ.  eps and the sharpness of the cases come from the reference alone (tests/test_host_pointing_ref.py).

Every test prints one line of figures ("pixels: ..."), the ones DESIGN 3.8a quotes."""

import ctypes as C
import functools

import numpy as np
import pointing_ref as pr
import pytest
import scipy.ndimage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = pr.cases()
case_param = pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
STORE_F32 = 2e-8    # rad: the float32 store of a value below 0.12
SAMPLER_F32 = 5e-8  # rad: the sampler's float32 map, weights and filter on values below 0.12
GAIN_SLACK = 1e-3   # pixels: the sampler's float32 gain product on indices up to 2043


@pytest.fixture(params=[0, 1], ids=["composed", "chain"])
def pointing_mode(request, gpu_ctx):
    """Both forms of steps 1-3: the composed float64 rotation (default) and the float32 chain (MRX_OPT_POINTING_CHAIN)."""
    gpu_ctx.set_option(0, request.param)
    yield ("composed", "chain")[request.param]
    gpu_ctx.set_option(0, 0)


def _t(a, dtype):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _device(case):
    """The case's pointing on the device, as every operator takes it."""
    t, az, el, off, transform, centre = case.inputs
    return dict(az=_t(az, np.float32), el=_t(el, np.float32), dx=_t(off[:, 0], np.float32), dy=_t(off[:, 1], np.float32),
                sw=_t(np.ones((len(off), 1)), np.float64), tr=None if transform is None else _t(transform.reshape(-1, 9), np.float64))


def _sky(case, bilinear):
    from maria_amd._lib import MrxSkyMap

    centre = case.inputs[5]
    return MrxSkyMap(None, 1, 1, case.eta.n, case.xi.n, case.eta.first, case.eta.step, case.xi.first, case.xi.step, centre[0], centre[1],
                     int(bilinear), 0)


def _point(case):
    """az, el, T, transform, dx, dy, stokes weights, channel (none), D"""
    from maria_amd._lib import ptr

    d = _device(case)
    D, T = case.exact.shape[:2]
    return (ptr(d["az"]), ptr(d["el"]), T, ptr(d["tr"]), ptr(d["dx"]), ptr(d["dy"]), ptr(d["sw"]), None, D)


def _planes(case, kind, dtype):
    """Two maps [n_eta, n_xi] on the device: every pixel's own (column, row) index, or its own (xi, eta) coordinate."""
    import torch

    if kind == "index":
        col, row = torch.arange(case.xi.n, dtype=dtype, device=DEV), torch.arange(case.eta.n, dtype=dtype, device=DEV)
    else:
        col, row = _t(case.xi.nodes, np.float64).to(dtype), _t(case.eta.nodes, np.float64).to(dtype)
    shape = (case.eta.n, case.xi.n)
    return col[None, :].expand(shape).contiguous(), row[:, None].expand(shape).contiguous()


def _project(ctx, case, bilinear, kind):
    """mrx_map_project of the two maps of _planes (float64): [2, D, T] float64 on the host, (along xi, along eta)."""
    import torch

    from maria_amd._lib import ptr

    D, T = case.exact.shape[:2]
    out = []
    for x in _planes(case, kind, torch.float64):
        y = torch.full((D, T), float("nan"), dtype=torch.float32, device=DEV)
        ctx.call("mrx_map_project", C.byref(_sky(case, bilinear)), ptr(x), *_point(case), 1.0, 0.0, ptr(y), y.stride(0))
        out.append(y.cpu().numpy().astype(np.float64))
    return np.stack(out)


def _sample(ctx, case, bilinear, kind):
    """mrx_map_sample of the two maps of _planes (float32) at unit gain: [2, D, T] float64 on the host."""
    import torch

    from maria_amd import map as mmap
    from oracle import mapsample

    t, az, el, off, transform, centre = case.inputs
    out = []
    for x in _planes(case, kind, torch.float32):
        y = mmap.sample_map(ctx, x[None, None], case.eta.nodes, case.xi.nodes, centre, az, el, off, np.ones((len(off), 1)), transform=transform,
                            bilinear=bilinear, cal_scalars=[1.0 / (1e12 * mapsample.K_B)])
        out.append(y.cpu().numpy().astype(np.float64))
    return np.stack(out)


def _filter(x):
    """The sampler's [0.25, 0.5, 0.25] along time, ends as scipy reflects them (oracle.mapsample.sample_maps)."""
    return scipy.ndimage.convolve1d(np.asarray(x, np.float64), weights=np.array([0.25, 0.5, 0.25]), axis=-1)


def _worst(case, ok):
    """Where the first failing sample is and how far it lies from the nearest pixel edge, for the assertion's message."""
    if ok.all():
        return ""
    d, s = np.argwhere(~ok)[0]
    u_eta = (case.exact[d, s, 1] - case.eta.first) / case.eta.step + 0.5
    u_xi = (case.exact[d, s, 0] - case.xi.first) / case.xi.step + 0.5
    edge = lambda u: abs(u - np.round(u))  # noqa: E731
    return (f"{int((~ok).sum())} samples outside their accepted set; first: detector {d} sample {s}, {edge(u_eta) * case.pixel:.3e} rad from an "
            f"eta edge, {edge(u_xi) * case.pixel:.3e} rad from a xi edge (eps {case.eps:.3e})")


@case_param
def test_project_names_an_accepted_pixel(gpu_ctx, case, pointing_mode):
    """mrx_map_project, nearest pixel, of the column-index and the row-index map: whole numbers, and every sample's (row,
    column) in its accepted set.  The kernel names its pixel by axis_weights (ml_corners: the float32 split form), as the
    binning does.  Printed, not asserted: on which member of a two-pixel set the samples fall."""
    cols, rows = _project(gpu_ctx, case, False, "index")
    assert np.isfinite(rows).all() and np.isfinite(cols).all()
    assert (rows == np.round(rows)).all() and (cols == np.round(cols)).all()
    lo_e, hi_e, lo_x, hi_x = case.sets
    ok = pr.check_pixels(rows, cols, lo_e, hi_e, lo_x, hi_x)
    two_e, two_x = hi_e > lo_e, hi_x > lo_x
    print(f"\npixels: project nearest  case {case.name} {pointing_mode}: eps {case.eps:.3e}; two-pixel sets (upper / lower index): "
          f"eta {int((rows == hi_e)[two_e].sum())} / {int((rows == lo_e)[two_e].sum())}, "
          f"xi {int((cols == hi_x)[two_x].sum())} / {int((cols == lo_x)[two_x].sum())}; outside {int((~ok).sum())} of {ok.size}")
    assert ok.all(), _worst(case, ok)


@case_param
def test_project_bilinear_returns_the_offsets(gpu_ctx, case, pointing_mode):
    """mrx_map_project, bilinear, of the maps of their own xi and eta coordinate (float64): the exact offset clipped to the
    axis' ends, within eps + 2e-8 (the float32 store) -- cell and weight together, on every sample."""
    got = _project(gpu_ctx, case, True, "ramp")
    err = np.abs(got - np.moveaxis(case.clipped, -1, 0))
    print(f"\npixels: project bilinear case {case.name} {pointing_mode}: max |device - exact| xi {err[0].max():.3e} eta {err[1].max():.3e} rad; "
          f"eps {case.eps:.3e}")
    assert np.isfinite(got).all() and err.max() <= case.eps + STORE_F32, np.argwhere(err > case.eps + STORE_F32)[:5]


@case_param
def test_sampler_bilinear_returns_the_filtered_offsets(gpu_ctx, case, pointing_mode):
    """mrx_map_sample at unit gain, bilinear, of the same ramps in float32: the [0.25, 0.5, 0.25] filter along time of the
    clipped exact offsets, within eps + 5e-8."""
    got = _sample(gpu_ctx, case, True, "ramp")
    err = np.abs(got - _filter(np.moveaxis(case.clipped, -1, 0)))
    print(f"\npixels: sampler bilinear case {case.name} {pointing_mode}: max |device - exact| xi {err[0].max():.3e} eta {err[1].max():.3e} rad; "
          f"eps {case.eps:.3e}")
    assert np.isfinite(got).all() and err.max() <= case.eps + SAMPLER_F32, np.argwhere(err > case.eps + SAMPLER_F32)[:5]


@case_param
def test_sampler_nearest_stays_between_the_accepted_pixels(gpu_ctx, case, pointing_mode):
    """mrx_map_sample at unit gain, nearest pixel, of the index maps: per axis between the filtered lowest and the filtered
    highest accepted index (1e-3 pixel for the float32 gain product).  The sampler's nearest pixel is axis_cell_t<false>, a
    float64 floor no other operator uses: this is the hold on it."""
    cols, rows = _sample(gpu_ctx, case, False, "index")
    lo_e, hi_e, lo_x, hi_x = case.sets
    out = 0
    for name, got, lo, hi in (("eta", rows, lo_e, hi_e), ("xi", cols, lo_x, hi_x)):
        bad = ~((got >= _filter(lo) - GAIN_SLACK) & (got <= _filter(hi) + GAIN_SLACK))
        out += int(bad.sum())
    print(f"\npixels: sampler nearest  case {case.name} {pointing_mode}: outside {out} of {2 * rows.size}")
    assert np.isfinite(rows).all() and np.isfinite(cols).all() and out == 0, np.argwhere(bad)[:5]


@functools.lru_cache(maxsize=None)
def _counts(case):
    """Per pixel [n_eta, n_xi]: the samples whose accepted set is that pixel alone, and those whose set contains it."""
    lo_e, hi_e, lo_x, hi_x = case.sets
    n = case.eta.n * case.xi.n
    single = (lo_e == hi_e) & (lo_x == hi_x)
    must = np.bincount((lo_e * case.xi.n + lo_x)[single], minlength=n)
    may = np.zeros(n, np.int64)
    for de in (0, 1):
        for dx in (0, 1):
            m = (de <= hi_e - lo_e) & (dx <= hi_x - lo_x)
            may += np.bincount(((lo_e + de) * case.xi.n + lo_x + dx)[m], minlength=n)
    assert (hi_e - lo_e).max() <= 1 and (hi_x - lo_x).max() <= 1 and (must <= may).all() and may.sum() > must.sum() == single.sum()
    shape = (case.eta.n, case.xi.n)
    return must.reshape(shape), may.reshape(shape)


@pytest.mark.parametrize("form", ["atomic", "routed_full", "routed_min"])
@case_param
def test_binning_counts_every_sample_in_an_accepted_pixel(gpu_ctx, case, form, pointing_mode):
    """mrx_bin_map and mrx_bin_map_bucketed (whole work buffer, and the sizing function's minimum: the time axis in chunks),
    nearest pixel, a TOD of ones, no weights: every pixel's weight a whole number between the samples that must and the
    samples that may fall on it, sum = weight, and D T samples in all -- the ones beyond the edges on the edge pixels.  Both
    forms name their cell by axis_weights, the routed one through bin_corners' region and pixel-in-region words."""
    import torch

    from maria_amd._lib import ptr

    D, T = case.exact.shape[:2]
    sky = _sky(case, False)
    tod = torch.ones((D, T), dtype=torch.float32, device=DEV)
    msum = torch.zeros((1, 1, case.eta.n, case.xi.n), dtype=torch.float64, device=DEV)
    mwgt = torch.zeros_like(msum)
    args = (C.byref(sky), ptr(tod), tod.stride(0), None, 0, *_point(case), ptr(msum), ptr(mwgt))
    if form == "atomic":
        gpu_ctx.call("mrx_bin_map", *args)
    else:
        lo, full = C.c_size_t(), C.c_size_t()
        assert gpu_ctx.lib.mrx_bin_map_work_bytes(C.byref(sky), D, T, C.byref(lo), C.byref(full)) == 0
        assert full.value == 3 * lo.value  # ceil(3001 / 1024) columns of tiles
        work = torch.empty(full.value if form == "routed_full" else lo.value, dtype=torch.uint8, device=DEV)
        gpu_ctx.call("mrx_bin_map_bucketed", *args, ptr(work), work.numel())
    torch.cuda.synchronize()
    wgt, total = mwgt[0, 0].cpu().numpy(), msum[0, 0].cpu().numpy()
    must, may = _counts(case)
    low, high = int((wgt < must).sum()), int((wgt > may).sum())
    print(f"\npixels: binning {form} case {case.name} {pointing_mode}: pixels below their least count {low}, above their largest {high}; "
          f"total {wgt.sum():.0f} of {D * T}")
    assert (wgt == np.round(wgt)).all() and np.array_equal(total, wgt)
    assert low == 0 and high == 0
    assert wgt.sum() == D * T
