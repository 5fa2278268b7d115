"""Band powers on the device: mrx_map_band_powers against the float64 oracle of tests/bandpower_ref.py on
modes made on the host, its bits from call to call, maria_amd.bandpowers.modes + the kernel against numpy's rfft2 + the
oracle, and the loop CMB.generate -> band_powers -> expected closed."""

import ctypes as C

import numpy as np
import pytest

import bandpower_ref as ref

pytestmark = pytest.mark.gpu

ARCMIN = np.radians(1.0 / 60.0)
RES = 2 * ARCMIN
SHAPES = [(8, 8), (16, 64), (64, 128), (32, 512), (48, 80), (128, 64)]  # rows of 5, 33, 65, 257, 41 and 33 cells

# the largest |device - oracle| / sum w |terms| of test_modes_and_kernel_against_numpy_rfft2, measured on an MI355X
E2E_MEASURED = 5.6e-16


def _edges(ny, nx, kind):
    """"uniform": 0 to past the plane's corner, nothing dropped but k = 0 and the Nyquist lines.  "cut": a first edge
    above the lowest cells, a last edge inside the plane, and behind the sixth edge a bin a thousandth of the cell
    spacing wide, which holds no cell."""
    step = 2 * np.pi / (max(ny, nx) * RES)
    if kind == "uniform":
        return np.linspace(0.0, 1.02 * np.pi * np.sqrt(2) / RES, 14)
    e = np.linspace(1.37 * step, 0.83 * np.pi / RES, 13)
    return np.sort(np.append(e, e[5] + 1e-3 * step))


def _host_modes(ny, nx, seed):
    """complex128 modes [3, ny, nx/2 + 1] whose amplitude falls by six decades from l = 0 to the plane's corner."""
    rng = np.random.default_rng(seed)
    l2 = ref.cells(ny, nx, RES, [0.0, 1.0])[0]
    amp = 10.0 ** (-6.0 * np.sqrt(l2) / (np.pi * np.sqrt(2) / RES))
    shape = (3, ny, nx // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * amp


def _call(ctx, a1, a2, ny, nx, res, edges, work=None, fill=None):
    """The C entry on device tensors -> (sums [n_bins, 8] on the host, the work buffer)."""
    import torch

    from maria_amd import _lib
    from maria_amd._lib import ptr

    edges = np.ascontiguousarray(edges, np.float64)
    n_bins = len(edges) - 1
    need = C.c_size_t()
    assert _lib.load().mrx_band_power_work_bytes(ny, nx, n_bins, C.byref(need)) == _lib.MRX_OK
    if work is None:
        work = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=a1.device)
    if fill is not None:
        work.fill_(fill)
    out = torch.full((n_bins, 8), float("nan"), dtype=torch.float64, device=a1.device)
    ctx.call("mrx_map_band_powers", ptr(a1), ptr(a2), ny, nx, float(res), edges.ctypes.data_as(C.POINTER(C.c_double)), n_bins,
             ptr(out), ptr(work), need.value)
    return out.cpu().numpy(), work


def _to_device(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def _assert_sums(got, want, scale, what):
    assert np.array_equal(got[:, 0], want[:, 0]), f"{what}: sum w"
    assert (np.abs(got[:, 1] - want[:, 1]) <= 1e-12 * np.abs(want[:, 1])).all(), f"{what}: sum w l"
    ratio = np.abs(got[:, 2:] - want[:, 2:]) / np.where(scale > 0, scale, 1.0)
    print(f"{what}: largest |device - oracle| / sum w |terms| = {ratio.max():.2e}")
    assert (np.abs(got[:, 2:] - want[:, 2:]) <= 1e-11 * scale).all(), what


@pytest.mark.parametrize("form", ["auto", "cross"])
@pytest.mark.parametrize("kind", ["uniform", "cut"])
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_kernel_against_the_oracle(gpu_ctx, ny, nx, kind, form):
    """sum w exactly, sum w l to 1e-12, every power column within 1e-11 x the oracle's sum w |terms| of its bin: a term
    carries about ten float64 roundings and a sum of n <= 1e4 terms adds n 2^-53, together below 2e-12.  Rows below, at
    and across a wave's 64 lanes, one shape that is no power of two, an empty bin, cells dropped on both sides."""
    edges = _edges(ny, nx, kind)
    l2, _, _, _, b = ref.cells(ny, nx, RES, edges)
    ell = np.sqrt(l2[b >= 0])
    assert ell.size and (np.abs(ell[:, None] - edges[None, :]) > 1e-9 * edges[None, :]).all()  # else: move the edges
    a1 = _host_modes(ny, nx, 1000 + ny + nx)
    a2 = a1 if form == "auto" else _host_modes(ny, nx, 2000 + ny + nx)
    want, scale = ref.sums(a1, a2, RES, edges)
    if kind == "cut":
        inner = np.delete(np.delete(l2, ny // 2, axis=0), nx // 2, axis=1)  # off the Nyquist lines
        inner = inner[inner > 0]
        assert want[5, 0] == 0 and (inner < edges[0] ** 2).any() and (inner >= edges[-1] ** 2).any()
    d1 = _to_device(a1)
    d2 = d1 if form == "auto" else _to_device(a2)
    got, _ = _call(gpu_ctx, d1, d2, ny, nx, RES, edges)
    _assert_sums(got, want, scale, f"{ny}x{nx} {kind} {form}")
    if kind == "cut":
        assert not got[5].any()


def test_two_calls_agree_bit_for_bit_whatever_the_work_buffer_held(gpu_ctx):
    ny, nx = 48, 80
    edges = _edges(ny, nx, "cut")
    d1, d2 = _to_device(_host_modes(ny, nx, 5)), _to_device(_host_modes(ny, nx, 6))
    first, work = _call(gpu_ctx, d1, d2, ny, nx, RES, edges, fill=0.0)
    again, _ = _call(gpu_ctx, d1, d2, ny, nx, RES, edges, work=work)
    poisoned, _ = _call(gpu_ctx, d1, d2, ny, nx, RES, edges, work=work, fill=float("nan"))
    assert np.isfinite(first).all() and first[:, 2:].any()
    assert first.tobytes() == again.tobytes() == poisoned.tobytes()


def test_modes_and_kernel_against_numpy_rfft2(gpu_ctx):
    """A 96 x 160 patch of a 256 x 512 CMB domain under taper(..., 0.2): bandpowers.modes + the kernel against numpy's
    rfft2 + the oracle.  What is left is the float64 transform's rounding, which moves from box to box: the bound is four
    times the largest |device - oracle| / sum w |terms| measured on an MI355X (E2E_MEASURED)."""
    from maria_amd import bandpowers as bp
    from maria_amd import cmb

    ny, nx = 96, 160
    sky = cmb.CMB.generate(width=((nx - 1) * 2.0 / 60, (ny - 1) * 2.0 / 60), resolution=2.0 / 60, spectrum=cmb.toy_spectrum(9000, r=0.05),
                           seed=31, domain=(256, 512), ctx=gpu_ctx)
    tqu = sky.data[:, 0, ::-1].astype(np.float64)
    assert tqu.shape == (3, ny, nx)
    win = bp.taper(ny, nx, 0.2)
    edges = bp.bin_edges(100, 200, 5300)
    m = bp.modes(tqu, win, RES)
    got = bp.binned_sums(m, m, edges, ctx=gpu_ctx)
    a, w = ref.modes(tqu, win, RES)
    want, scale = ref.sums(a, a, RES, edges)
    np.testing.assert_array_equal(m.window.cpu().numpy(), w)
    assert np.array_equal(got[:, 0], want[:, 0]) and (want[:, 0] > 0).all()
    ratio = float((np.abs(got[:, 2:] - want[:, 2:]) / scale).max())
    print(f"modes + kernel against numpy rfft2 + oracle: largest |device - oracle| / sum w |terms| = {ratio:.3e}")
    assert E2E_MEASURED <= 2.5e-9  # four times it stays below 1e-8: more would be a finding, not a bound to raise
    assert ratio <= 4 * E2E_MEASURED


def test_the_loop_closes_on_a_periodic_patch(gpu_ctx):
    """CMB.generate with domain = the map (periodic, unit window) -> band_powers of the ProjectionMap: every bin with
    N_b = n_modes / 2 >= 400 cells within 5 / sqrt(N_b) of expected(spectrum) in TT and EE, and no B: BB / EE < 1e-10
    (the maps are float32)."""
    from maria_amd import bandpowers as bp
    from maria_amd import cmb

    n = 256
    sky = cmb.CMB.generate(width=(n - 1) * 2.0 / 60, resolution=2.0 / 60, spectrum=cmb.toy_spectrum(9000), seed=21, domain=n, ctx=gpu_ctx)
    got = bp.band_powers(sky, edges=bp.bin_edges(100, 200, 7700), ctx=gpu_ctx)
    assert got.shape == (n, n) and got.res == pytest.approx(RES, rel=1e-12)
    want = bp.expected(sky.spectrum, got)
    np.testing.assert_array_equal(want, ref.expected(sky.spectrum, n, n, got.res, got.edges))
    n_b = got.n_modes / 2
    full = n_b >= 400
    assert full.sum() >= 15
    for col, name in ((0, "TT"), (1, "EE")):
        dev = np.abs(got.cl[full, col] / want[full, col] - 1) * np.sqrt(n_b[full])
        print(f"{name}: largest |C_b / expected - 1| sqrt N_b = {dev.max():.2f}")
        assert dev.max() <= 5, name
    bb, ee = np.nansum(got.cl[:, 2] * got.n_modes), np.nansum(got.cl[:, 1] * got.n_modes)
    print(f"BB / EE = {bb / ee:.2e}")
    assert 0 <= bb < 1e-10 * ee
    # the same numbers as an array with res=: rows in ascending eta, as the generator made them
    as_array = bp.band_powers(sky.data[:, 0, ::-1], edges=got.edges, res=got.res, ctx=gpu_ctx)
    assert as_array.cl.tobytes() == got.cl.tobytes()
    # I alone gives the same TT
    only_t = bp.band_powers(sky.data[:1, 0, ::-1], edges=got.edges, res=got.res, ctx=gpu_ctx)
    assert only_t.cl[:, 0].tobytes() == got.cl[:, 0].tobytes() and not np.nan_to_num(only_t.cl[:, 1:]).any()


def test_transfer_function_and_window_from_weight(gpu_ctx):
    """Outputs that are half their inputs have the transfer function 1/2 in every column that holds power, and dividing
    by it gives the inputs' spectra back; window_from_weight of a disc of hits is 1 deep inside, below 0.05 from the disc's
    edge outwards, 0 beyond the stencil's reach, and falls monotonically in between along a radius; with hits that fill
    the map it falls to the map's border as well."""
    from maria_amd import bandpowers as bp

    rng = np.random.default_rng(2)
    ny, nx = 64, 96
    ins = [rng.standard_normal((3, ny, nx)) for _ in range(2)]
    outs = [0.5 * m for m in ins]
    win = bp.taper(ny, nx, 0.3)
    kw = dict(edges=bp.bin_edges(300, 600, 5000), window=win, res=RES, ctx=gpu_ctx)
    tf = bp.transfer_function(ins, outs, **kw)
    assert tf.shape == (7, 6) and np.abs(tf - 0.5).max() <= 1e-12
    back = bp.band_powers(outs[0], outs[0], transfer=tf**2, **kw)
    np.testing.assert_allclose(back.cl, bp.band_powers(ins[0], **kw).cl, rtol=1e-10, atol=0)
    yy, xx = np.mgrid[:128, :128]
    r = np.hypot(yy - 63.5, xx - 63.5)
    weight = np.where(r < 50, 5.0 + rng.uniform(0, 1, r.shape), 0.0)
    weight[r >= 50] = np.nan
    sigma = 4.0
    w = bp.window_from_weight(weight, sigma, ctx=gpu_ctx)
    assert w.shape == (128, 128) and w.dtype == np.float64 and w.min() >= 0 and w.max() <= 1
    # the first smoothing and the 0.99 cut move the edge at least 2 sigma inwards; the second spreads it over the stencil's
    # square of +- 4 sigma, 4 sqrt 2 sigma + a pixel along a diagonal
    assert (w[r >= 50] < 0.05).all() and not w[r > 50 + 4 * sigma].any()
    assert (w[r < 50 - 7 * sigma] > 0.999).all()
    line = w[64, 64:]
    assert (np.diff(line) <= 1e-5).all() and line[0] > 0.999 and line[-1] == 0
    # hits that fill the map: its border is an edge of the coverage too, the window falls to it on all four sides
    filled = bp.window_from_weight(np.full((96, 128), 3.0), sigma, ctx=gpu_ctx)
    rim = np.concatenate([filled[0], filled[-1], filled[:, 0], filled[:, -1]])
    assert rim.max() < 0.05 and filled[48, 64] > 0.999 and (np.diff(filled[48, :64]) >= -1e-5).all()


def test_refusals(gpu_ctx):
    from maria_amd import _lib
    from maria_amd import bandpowers as bp
    from maria_amd._lib import MrxError, ptr

    ny, nx = 16, 32
    d = _to_device(_host_modes(ny, nx, 1))
    good = np.array([0.0, 1000.0, 2000.0])
    for bad_ny, bad_nx in ((15, 32), (16, 31), (6, 32), (16, 4)):
        with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
            gpu_ctx.call("mrx_map_band_powers", ptr(d), ptr(d), bad_ny, bad_nx, RES, good.ctypes.data_as(C.POINTER(C.c_double)), 2, ptr(d), ptr(d), 1 << 30)
        assert _lib.load().mrx_band_power_work_bytes(bad_ny, bad_nx, 2, C.byref(C.c_size_t())) != _lib.MRX_OK
    for edges in ([0.0, 2000.0, 1000.0], [0.0, 1000.0, 1000.0], [-1.0, 1000.0, 2000.0], [0.0, 1000.0, np.nan]):
        with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
            _call(gpu_ctx, d, d, ny, nx, RES, np.array(edges))
    for res in (0.0, -RES, float("nan")):
        with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
            _call(gpu_ctx, d, d, ny, nx, res, good)
    import torch

    need = C.c_size_t()
    assert _lib.load().mrx_band_power_work_bytes(ny, nx, 2, C.byref(need)) == _lib.MRX_OK
    assert need.value >= 8 * (3 + ny * 2 * 8)
    for n_bins in (0, 1025):
        assert _lib.load().mrx_band_power_work_bytes(ny, nx, n_bins, C.byref(C.c_size_t())) != _lib.MRX_OK
        many = np.arange(1027.0)
        with pytest.raises(MrxError, match="n_bins"):
            gpu_ctx.call("mrx_map_band_powers", ptr(d), ptr(d), ny, nx, RES, many.ctypes.data_as(C.POINTER(C.c_double)), n_bins, ptr(d), ptr(d), 1 << 30)
    out = torch.empty((2, 8), dtype=torch.float64, device="cuda:0")
    work = torch.empty(need.value // 8, dtype=torch.float64, device="cuda:0")
    e = good.ctypes.data_as(C.POINTER(C.c_double))
    with pytest.raises(MrxError, match="work buffer"):
        gpu_ctx.call("mrx_map_band_powers", ptr(d), ptr(d), ny, nx, RES, e, 2, ptr(out), ptr(work), need.value - 1)
    for args in ((None, ptr(d), ny, nx, RES, e, 2, ptr(out), ptr(work), need.value), (ptr(d), None, ny, nx, RES, e, 2, ptr(out), ptr(work), need.value),
                 (ptr(d), ptr(d), ny, nx, RES, None, 2, ptr(out), ptr(work), need.value), (ptr(d), ptr(d), ny, nx, RES, e, 2, None, ptr(work), need.value),
                 (ptr(d), ptr(d), ny, nx, RES, e, 2, ptr(out), None, need.value)):
        with pytest.raises(MrxError, match="null pointer"):
            gpu_ctx.call("mrx_map_band_powers", *args)
    # band_powers' own argument errors
    m = np.zeros((3, ny, nx))
    with pytest.raises(ValueError, match="shape"):
        bp.band_powers(m, np.zeros((3, ny, nx + 2)), edges=good, res=RES, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="window"):
        bp.band_powers(m, window=np.ones((ny, nx + 2)), edges=good, res=RES, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="ascending"):
        bp.band_powers(m, edges=[0.0, 2000.0, 1000.0], res=RES, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="res"):
        bp.band_powers(m, edges=good)
    with pytest.raises(ValueError, match="even"):
        bp.band_powers(np.zeros((3, 15, 32)), edges=good, res=RES, ctx=gpu_ctx)
