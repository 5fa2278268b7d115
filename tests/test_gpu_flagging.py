"""mrx_tod_median_residual, mrx_tod_glitch_flag, mrx_tod_gap_fill, maria_amd.flagging and the flags' way through TOD and
the mappers on the device, against the numpy / scipy reference of tests/flagging_ref.py.

The median is a selection and the flags are comparisons of it: residuals, flags, counts and the robust scale are compared
bit for bit.  The gap fill is a float64 line rounded once to float32: |gpu - ref| <= 2^-23 max(|yL|, |yR|)."""

import flagging_ref as ref
import numpy as np
import pytest
from test_gpu_downsample import _centre, hand_tod

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 1  # of the glitches of test_the_map_through_glitches


def S():
    from maria_amd import flagging

    return flagging.TILE_SAMPLES


def lengths(h):
    s = S()
    return [1, 2, h, 2 * h, 2 * h + 1, s - 1, s, s + 1, 2 * s + h + 3, 3 * s + 17]


def tied_rows(D, T, seed=0):
    """Noise plus a drift, every seventh sample set to the row's first: ties in every window."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((D, T)) + np.linspace(0.0, 3.0, T) + 5).astype(np.float32)
    x[:, ::7] = x[:, :1]
    return x


def device_rows(a, pitch, offset, fill):
    """The [D, T] array ``a`` on the device at row pitch ``pitch``, ``offset`` elements into a buffer filled with ``fill``:
    (buffer, view)."""
    import torch

    a = np.asarray(a)
    D, T = a.shape
    buf = torch.full((offset + D * pitch + 64,), fill, dtype=torch.as_tensor(a[:0]).dtype, device=DEV)
    view = torch.as_strided(buf, (D, T), (pitch, 1), offset)
    view.copy_(torch.as_tensor(a))
    return buf, view


def untouched_outside(buf, view, fill):
    """Was nothing but the view written?  (Fills the view; call after reading it.)"""
    view.fill_(fill)
    return bool((buf == fill).all())


@pytest.mark.parametrize("D", [1, 3, 65])
@pytest.mark.parametrize("h", [1, 5, 15])
def test_residual_bit_for_bit(gpu_ctx, h, D):
    import torch

    from maria_amd import flagging

    for T in lengths(h):
        x = tied_rows(D, T, seed=T + D)
        want, _ = ref.median_residual(x, h)
        xbuf, xv = device_rows(x, T + 3, 1, -3.0)  # a padded pitch and an odd element offset
        before = xbuf.clone()
        rbuf, rv = device_rows(np.zeros_like(x), T + 5, 0, 7.0)
        rv.fill_(7.0)
        out = flagging.median_residual(xv, h, ctx=gpu_ctx, out=rv)
        torch.cuda.synchronize()
        assert out is rv and torch.equal(xbuf, before), "the input changed"
        got = rv.cpu().numpy()
        assert np.array_equal(got, want), (T, int((got != want).sum()))
        assert untouched_outside(rbuf, rv, 7.0), "written past T"
    assert np.array_equal(flagging.median_residual(torch.as_tensor(x).to(DEV), h, ctx=gpu_ctx).cpu().numpy(), want)  # out=None


def flag_case(D, T, h, grow, seed):
    """(x, thresh): tied rows with hand-placed spikes, thresholds at each row's 99.5th percentile of |r| (0.1 - 1 % of a
    long row are detections).  The spikes sit at 0, 1, T - 2, T - 1, S - 1, S and S + grow_after of row 0 (its last row
    too), so that growing crosses tile seams and row ends.  By the edge rule the window of sample 0 holds it h + 1 times:
    r[0] = r[T - 1] = 0 whatever the data, and the spikes at 1 and T - 2 are the detections next to the ends."""
    s = S()
    x = tied_rows(D, T, seed=seed)
    for t in (0, 1, T - 2, T - 1, s - 1, s, s + grow[1]):
        if 0 <= t < T:
            x[0, t] += 40.0
            if D > 1:
                x[-1, t] -= 40.0
    if D > 2:
        x[1] = 2.5  # a row of constants: with thresh = 0 it flags nothing
    r, _ = ref.median_residual(x, h)
    thresh = np.quantile(np.abs(r).astype(np.float64), 0.995, axis=1).astype(np.float32)
    if D > 2:
        thresh[1] = 0.0
    return x, thresh


def run_flags(gpu_ctx, x, h, thresh, grow, pad_f, off_f, count=True):
    """mrx_tod_glitch_flag into a sentinel-filled byte buffer at pitch T + pad_f, off_f bytes in: (flags, count)."""
    import torch

    from maria_amd._lib import ptr

    D, T = x.shape
    _, xv = device_rows(x, T + 1, 1, -3.0)
    fbuf, fv = device_rows(np.full((D, T), 9, np.uint8), T + pad_f, off_f, 9)
    d_thresh = torch.as_tensor(np.asarray(thresh, np.float32)).to(DEV)
    d_count = torch.full((D,), 12345, dtype=torch.int32, device=DEV)  # overwritten, not accumulated
    gpu_ctx.call("mrx_tod_glitch_flag", ptr(xv), T + 1, D, T, h, ptr(d_thresh), grow[0], grow[1], ptr(fv), T + pad_f,
                 ptr(d_count) if count else None)
    torch.cuda.synchronize()
    got = fv.cpu().numpy()
    assert untouched_outside(fbuf, fv, 9), "written outside the rows"
    return got, d_count.cpu().numpy()


@pytest.mark.parametrize("grow", [(0, 0), (2, 8), (64, 64), (0, 64)])
@pytest.mark.parametrize("h", [1, 5, 15])
def test_flags_and_counts_bit_for_bit(gpu_ctx, h, grow):
    s = S()
    for T in lengths(h):
        for D in (1, 3, 65):
            x, thresh = flag_case(D, T, h, grow, seed=T + D + h)
            want, n_want = ref.flags(x, h, thresh, *grow)
            if T >= s - 1:
                assert (want == 1).sum() > 0 and (want == 1).mean() < 0.011  # the reference has detections, and few
                if D > 2:
                    assert not want[1].any()
            # word stores: pitch and base multiples of 4; byte stores: an odd pitch and an odd base
            aligned = (4 - T % 4) % 4, 0
            for pad_f, off_f in (aligned, (aligned[0] + 1, 3)):
                got, n_got = run_flags(gpu_ctx, x, h, thresh, grow, pad_f, off_f)
                assert np.array_equal(got, want), (T, D, pad_f, int((got != want).sum()))
                assert np.array_equal(n_got, n_want), (T, D, pad_f)


def test_flags_without_a_count_and_with_every_sample_detected(gpu_ctx):
    """d_count = NULL is allowed; a negative threshold (the C entry takes it, the Python layer does not) detects every
    sample, the row ends included."""
    T = 2 * S() + 9
    x = tied_rows(2, T, seed=4)
    got, n = run_flags(gpu_ctx, x, 5, [-1.0, np.inf], (3, 3), 0, 1, count=False)
    assert (got[0] == 1).all() and not got[1].any() and (n == 12345).all()
    got, n = run_flags(gpu_ctx, x, 5, [-1.0, np.inf], (3, 3), 0, 1)
    assert n.tolist() == [T, 0]


def test_robust_sigma_in_three_chunks(gpu_ctx):
    import torch

    from maria_amd import flagging

    D, T = 70, 2 * S() + 5
    x = tied_rows(D, T, seed=6)
    x[:, 100:103] += 50.0  # a glitch (shorter than the half window) does not move the scale
    xd = torch.as_tensor(x).to(DEV)
    got = flagging.robust_sigma(xd, 5, ctx=gpu_ctx, scratch_bytes=4 * T * 30 + 17)  # 30 + 30 + 10 rows
    assert got.dtype == torch.float64 and tuple(got.shape) == (D,)
    want = ref.robust_sigma(x, 5)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(flagging.robust_sigma(xd, 5, ctx=gpu_ctx).cpu().numpy(), want)  # one chunk
    # find_glitches with and without a given sigma: the reference's flags at float32(n_sigma * sigma)
    f_want, n_want = ref.flags(x, 5, (6.0 * want).astype(np.float32), 2, 8)
    assert n_want.min() >= 10
    for sigma in (None, want, got):
        f, n = flagging.find_glitches(xd, 6.0, 5, (2, 8), sigma=sigma, ctx=gpu_ctx)
        assert f.dtype == torch.uint8 and n.dtype == torch.int64
        np.testing.assert_array_equal(f.cpu().numpy(), f_want)
        np.testing.assert_array_equal(n.cpu().numpy(), n_want)


def fill_case(n_fit, seed=0, dyadic=False):
    """(x, flags) of 5 rows of T = 4 S + 37: row 0 runs of length 1, 2, n_fit and S + 3 (across a seam), one at t = 0, one
    ending at T, and two runs one unflagged sample apart; row 1 a run of 3 S; row 2 flagged end to end; row 3 none; row 4
    random flags of both values."""
    s = S()
    T = 4 * s + 37
    rng = np.random.default_rng(seed)
    if dyadic:
        x = (rng.integers(-(1 << 14) + 1, 1 << 14, (5, T)) / 64.0).astype(np.float32)  # multiples of 2^-6 below 2^8
    else:
        x = (rng.standard_normal((5, T)) * 3 + np.linspace(-20.0, 20.0, T)).astype(np.float32)
    f = np.zeros((5, T), np.uint8)
    for a, n in ((0, 3), (10, 1), (20, 2), (40, n_fit), (100, 3), (104, 2), (s - 10, s + 3), (T - 5, 5)):
        f[0, a:a + n] = 1 + (a % 2)
    f[1, 50:50 + 3 * s] = 2
    f[2] = 1
    f[4] = (rng.random(T) < 0.02) * rng.integers(1, 3, T)
    return x, f


def run_fill(gpu_ctx, x, f, n_fit, pad_x, pad_f, off_f):
    import torch

    from maria_amd import flagging

    D, T = x.shape
    xbuf, xv = device_rows(x, T + pad_x, 1, -3.0)
    fbuf, fv = device_rows(f, T + pad_f, off_f, 0)
    f_before = fbuf.clone()
    filled = flagging.gap_fill(xv, fv, n_fit, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert torch.equal(fbuf, f_before), "the flags changed"
    got = xv.cpu().numpy()
    assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"
    return got, filled.cpu().numpy()


@pytest.mark.parametrize("n_fit", [1, 4, 16])
def test_gap_fill(gpu_ctx, n_fit):
    x, f = fill_case(n_fit, seed=n_fit)
    T = x.shape[1]
    want, n_want, scale = ref.gap_fill(x, f, n_fit)
    assert n_want[2] == 0 and n_want[3] == 0 and n_want[1] == 3 * S() and np.array_equal(want[2], x[2])
    for pad_f, off_f in (((4 - T % 4) % 4, 0), (0, 1)):  # flags read as words, and as bytes
        got, filled = run_fill(gpu_ctx, x, f, n_fit, 3, pad_f, off_f)
        keep = (f == 0) | (np.arange(5) == 2)[:, None]
        assert np.array_equal(got[keep], x[keep]), "an unflagged sample, or the row flagged end to end, changed"
        err = np.abs(got.astype(np.float64) - want)
        worst = float((err[~keep] / (2.0**-23 * scale[~keep])).max())
        print(f"n_fit {n_fit}: max |gpu - ref| / (2^-23 max(|yL|, |yR|)) = {worst:.3f}")
        assert worst <= 1.0
        assert np.array_equal(filled, n_want) and np.array_equal(filled, ((f != 0) & ~keep).sum(axis=1))


def test_gap_fill_is_exact_on_dyadic_inputs(gpu_ctx):
    """Single-sample anchors (n_fit = 1) of multiples of 2^-6 below 2^8: yL and yR are the samples themselves, the line is
    the reference's float64 expression operation by operation, and the fill is equal bit for bit."""
    x, f = fill_case(1, seed=9, dyadic=True)
    want, n_want, _ = ref.gap_fill(x, f, 1)
    got, filled = run_fill(gpu_ctx, x, f, 1, 0, 0, 0)
    assert np.array_equal(got, want) and np.array_equal(filled, n_want)


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T = 4, 3000
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    x[:, 1500] = 50.0
    x0 = x.clone()
    r = torch.full((D, T), 7.0, dtype=torch.float32, device=DEV)
    th = torch.zeros(D, dtype=torch.float32, device=DEV)
    f = torch.full((D, T), 9, dtype=torch.uint8, device=DEV)
    ones = torch.ones((D, T), dtype=torch.uint8, device=DEV)
    ones[:, 0] = 0
    n = torch.full((D,), 12345, dtype=torch.int32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    res = (ptr(x), T, D, T, 5, ptr(r), T)
    flag = (ptr(x), T, D, T, 5, ptr(th), 2, 8, ptr(f), T, ptr(n))
    fill = (ptr(x), T, D, T, ptr(ones), T, 4, ptr(n))

    def put(args, i, v):
        return args[:i] + (v,) + args[i + 1:]

    cases = {
        "mrx_tod_median_residual": {
            "null x": put(res, 0, None), "null r": put(res, 5, None), "D 0": put(res, 2, 0), "T 0": put(res, 3, 0),
            "ld_x < T": put(res, 1, T - 1), "ld_r < T": put(res, 6, T - 1), "h 0": put(res, 4, 0), "h 16": put(res, 4, 16),
            "r is x": put(res, 5, ptr(x)),
        },
        "mrx_tod_glitch_flag": {
            "null x": put(flag, 0, None), "null thresh": put(flag, 5, None), "null flags": put(flag, 8, None), "D 0": put(flag, 2, 0),
            "T 0": put(flag, 3, 0), "ld_x < T": put(flag, 1, T - 1), "ld_f < T": put(flag, 9, T - 1), "h 0": put(flag, 4, 0),
            "h 16": put(flag, 4, 16), "grow_before -1": put(flag, 6, -1), "grow_before 65": put(flag, 6, 65),
            "grow_after -1": put(flag, 7, -1), "grow_after 65": put(flag, 7, 65),
        },
        "mrx_tod_gap_fill": {
            "null x": put(fill, 0, None), "null flags": put(fill, 4, None), "D 0": put(fill, 2, 0), "T 0": put(fill, 3, 0),
            "ld_x < T": put(fill, 1, T - 1), "ld_f < T": put(fill, 5, T - 1), "n_fit 0": put(fill, 6, 0), "n_fit 17": put(fill, 6, 17),
        },
    }
    for entry, bad in cases.items():
        for name, args in bad.items():
            assert getattr(lib, entry)(hd, *args) == -1, (entry, name)
            assert entry.encode() in lib.mrx_last_error(hd), (entry, name)
    torch.cuda.synchronize()
    assert bool((r == 7.0).all()) and bool((f == 9).all()) and bool((n == 12345).all()) and torch.equal(x, x0)
    assert lib.mrx_tod_median_residual(hd, *res) == 0 and lib.mrx_tod_glitch_flag(hd, *flag) == 0
    assert n.tolist() == [11] * D and float(r[0, 1500]) == 49.0
    assert lib.mrx_tod_gap_fill(hd, *put(fill, 4, ptr(f))) == 0
    assert n.tolist() == [11] * D and bool((x == 1.0).all())


def test_tod_flag_glitches_to_and_downsample(gpu_ctx):
    import torch

    from maria_amd import flagging

    tod, _, _ = hand_tod()  # 6 x 3001: "map" a numpy field, "noise" a device field
    D, T = 6, 3001
    flagging.inject_glitches(tod.data["noise"], 3, (20.0, 200.0), 3.0, seed=5)
    tod._calibrator = lambda data, to_krj: data
    kept = {k: (v.clone() if isinstance(v, torch.Tensor) else v.copy()) for k, v in tod.data.items()}
    out = tod.flag_glitches(ctx=gpu_ctx)
    # the source is as it was
    assert tod.flags is None and "glitches" not in tod.metadata and isinstance(tod.data["map"], np.ndarray)
    for name, v in kept.items():
        assert torch.equal(tod.data[name], v) if isinstance(v, torch.Tensor) else np.array_equal(tod.data[name], v), name
    # the flags are the reference's on the float32 sum of the fields
    signal = kept["map"] + kept["noise"].cpu().numpy()
    f_want, n_want = ref.flags(signal, 5, (6.0 * ref.robust_sigma(signal, 5)).astype(np.float32), 2, 8)
    assert n_want.sum() >= 3 * D * 5
    assert out.flags.dtype == torch.uint8 and out.flags.is_cuda
    np.testing.assert_array_equal(out.flags.cpu().numpy(), f_want)
    g = out.metadata["glitches"]
    assert (g["n_sigma"], g["half_window"], g["grow"], g["n_fit"], g["fill"]) == (6.0, 5, (2, 8), 4, True)
    np.testing.assert_array_equal(g["counts"], n_want)
    assert g["flagged_fraction"] == n_want.sum() / (D * T) and out.metadata["latitude"] == -23.0
    assert out.dets is tod.dets and out.coords is tod.coords and out.units == tod.units and out._calibrator is tod._calibrator
    # every field gap-filled with the same flags
    assert out.fields == ["map", "noise"]
    for name in out.fields:
        v = out.data[name]
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32
        src = kept[name].cpu().numpy() if isinstance(kept[name], torch.Tensor) else kept[name]
        want, _, scale = ref.gap_fill(src, f_want, 4)
        err = np.abs(v.cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= 2.0**-23 * scale), name
    raw = tod.flag_glitches(fill=False, ctx=gpu_ctx)
    assert torch.equal(raw.flags, out.flags) and torch.equal(raw.data["noise"], kept["noise"]) and raw.data["noise"] is not tod.data["noise"]
    # flags the TOD already has are kept
    tod.flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    tod.flags[2, 7:9] = 1
    both = tod.flag_glitches(ctx=gpu_ctx)
    union = (f_want != 0) | (tod.flags.cpu().numpy() != 0)
    np.testing.assert_array_equal(both.flags.cpu().numpy() != 0, union)
    np.testing.assert_array_equal(both.metadata["glitches"]["counts"], union.sum(axis=1))
    # to() and downsample() carry them
    assert out.to("pW").flags is out.flags
    low = out.downsample(4, ctx=gpu_ctx)
    assert low.flags.dtype == torch.uint8 and tuple(low.flags.shape) == (D, 751)
    np.testing.assert_array_equal(low.flags.cpu().numpy(), ref.downsample_flags(f_want, 4))
    assert tod.downsample(4, ctx=gpu_ctx).flags is not None and hand_tod()[0].downsample(4, ctx=gpu_ctx).flags is None


def _flagged_pair(seed=3):
    """hand_tod's pointing with 31 detectors at polarisation angle 0 x 8001 samples of small integers, 1 % of them flagged
    by hand in runs of ten: (mask, data, make, centre az, el); make(value, flagged=True) is the TOD with ``value`` in the
    masked samples, with the mask as its flags or with none."""
    import torch

    tod, az, el = hand_tod(D=31, T=8001, seed=seed, gamma=0.0)
    rng = np.random.default_rng(seed)
    data = rng.integers(-64, 65, (31, 8001)).astype(np.float32)
    mask = np.zeros((31, 8001), bool)
    for d in range(31):
        for a in rng.choice(799, 8, replace=False) * 10 + 3:
            mask[d, a:a + 10] = True
    assert 0.009 < mask.mean() < 0.011

    def make(value, flagged=True):
        from maria_amd.sim import TOD

        return TOD({"map": np.where(mask, np.float32(value), data)}, tod.dets, tod.coords, units="K_RJ", metadata=dict(tod.metadata),
                   flags=torch.as_tensor(mask.astype(np.uint8) * 2).to(DEV) if flagged else None)

    return mask, data, make, az, el


def test_bin_mapper_gives_flagged_samples_no_weight_exactly(gpu_ctx):
    from maria_amd.map import mueller_row
    from maria_amd.mappers import BinMapper

    mask, data, make, az, el = _flagged_pair()
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="I", frame="az/el", units="K_RJ")
    assert np.all(mueller_row(make(0).dets.gamma)[:, 0] == 0.5)  # exact float64 sums in any order
    flagged = BinMapper([make(2.0**20)], **kw)
    plain = BinMapper([make(0.0, flagged=False)], **kw)
    flagged.run(), plain.run()
    assert np.abs(plain.products["sum"]).sum() > 0
    np.testing.assert_array_equal(flagged.products["sum"], plain.products["sum"])
    ones = make(0.0, flagged=False)
    ones.data = {"map": (~mask).astype(np.float32)}
    hits = BinMapper([ones], **kw)
    hits.run()
    np.testing.assert_array_equal(flagged.products["weight"], hits.products["sum"])
    assert (flagged.products["weight"] < plain.products["weight"]).any()


@pytest.mark.parametrize("case", ["ml", "ml bilinear", "ml noise_model", "destriper"])
def test_flagged_samples_do_not_move_the_gls_maps(gpu_ctx, case):
    """The map with 10^6 in the flagged samples against the map with -3 10^5 there, tol = 1e-9: within 1e-6 max|map|.
    One leaked sample in a pixel of <= 10^3 hits would move it by >= 1.3 10^3.  The nearest-pixel maps of these white
    data are O(10), the bound eight orders below a leak; the bilinear map's poorly determined edge pixels amplify white
    data to 10^6, and the bound stays three orders below (asserted: at most a hundredth of a leak)."""
    from maria_amd.mappers import DestripingMapper, MaximumLikelihoodMapper

    mask, data, make, az, el = _flagged_pair()
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="I", frame="az/el", units="K_RJ", tol=1e-9, max_iter=500)
    if case == "ml":
        build = lambda t: MaximumLikelihoodMapper([t], noise_weights="uniform", **kw)  # noqa: E731
    elif case == "ml bilinear":
        build = lambda t: MaximumLikelihoodMapper([t], noise_weights="uniform", bilinear=True, **kw)  # noqa: E731
    elif case == "ml noise_model":
        build = lambda t: MaximumLikelihoodMapper([t], noise_model={"white": 1.0, "knee": 0.5, "alpha": 1.0}, **kw)  # noqa: E731
    else:
        build = lambda t: DestripingMapper([t], noise_weights="uniform", **kw)  # noqa: E731
    maps = [build(make(v)).run().data.astype(np.float64) for v in (1e6, -3e5)]
    np.testing.assert_array_equal(np.isnan(maps[0]), np.isnan(maps[1]))
    ok = np.isfinite(maps[0])
    top = np.abs(maps[0][ok]).max()
    diff = np.abs(maps[0][ok] - maps[1][ok]).max()
    print(f"{case}: max|map| {top:.3g}, max difference {diff:.3g} ({diff / top:.2e} of it)")
    assert ok.sum() > 100 and top > 1e-2 and 1e-6 * top <= 1e-2 * 1.3e6 / 1e3 and diff <= 1e-6 * top


def test_noise_modes_refuse_a_flagged_tod(gpu_ctx):
    from maria_amd.mappers import MaximumLikelihoodMapper

    mask, data, make, az, el = _flagged_pair()
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="I", frame="az/el", units="K_RJ")
    with pytest.raises(ValueError, match="differ by row"):
        MaximumLikelihoodMapper([make(0.0)], noise_model="fit", noise_modes=1, **kw).run()
    given = {"white": 1.0, "knee": 0.5, "alpha": 1.0, "modes": np.ones((31, 1)), "mode_law": {"white": 1.0, "knee": 0.5, "alpha": 1.0}}
    with pytest.raises(ValueError, match="differ by row"):
        MaximumLikelihoodMapper([make(0.0)], noise_model=given, **kw).run()


def test_the_map_through_glitches(gpu_ctx):
    """test_gpu_downsample.py::test_recover_map_at_the_reduced_rate's set-up at 50 Hz (300 positions x 3 bands, a 60 s
    daisy, no atmosphere) plus white noise of sigma = 2e-4 K_RJ as a second field and one glitch a row (50 - 500 sigma of
    either sign, tau = 3 samples), binned on the input map's grid three times: clean, glitchy, glitchy.flag_glitches().
    With res the weighted rms residual per band against the input map: every onset is flagged, at most 2 % of the samples
    are, res(flagged) <= 1.1 res(clean) and res(glitchy) >= 3 res(clean).  (DESIGN 3.20 holds the three residuals.)

    By the median's edge rule r[0] = r[T - 1] = 0 whatever the data, and a glitch that starts on a row's first sample is a
    monotone run from the edge, which a running median follows: the seed is one whose onsets avoid the two end samples."""
    import torch

    from maria_amd import flagging
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.mappers import BinMapper
    from maria_amd.sim import TOD, Plan, Simulation, sky_transform_stack

    bands = [Band(center=90e9, width=30e9, name="f090"), Band(center=150e9, width=40e9, name="f150"), Band(center=220e9, width=50e9, name="f220")]
    n, width = 128, 1.0  # degrees
    res = width / (n - 1)
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    rng = np.random.default_rng(8)
    field = np.fft.irfft2(np.fft.rfft2(rng.standard_normal((n, n))) * np.exp(-0.5 * (np.hypot(*np.meshgrid(np.fft.rfftfreq(n), np.fft.fftfreq(n))) * 12.0) ** 2), s=(n, n))
    data = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0 + 4e-4 * field / field.std()
    data = (data - data.mean()).astype(np.float32)
    inst = Instrument(Detectors.hexagon(300, width / 2, bands, primary_size=1000.0))
    site = Site(altitude=5190.0)
    plan = Plan.daisy(start_time=1.7e9, duration=60.0, sample_rate=50.0, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
    centre = _centre(plan.phi.astype(np.float32), plan.theta.astype(np.float32), sky_transform_stack(plan.time, site.latitude, site.longitude))
    sky = mmap.ProjectionMap(data, nu=150e9, width=width, center=np.degrees(centre), frame="ra/dec")
    (clean,) = Simulation(inst, plan, site, map=sky, noise=False).run()
    assert clean.units == "K_RJ" and set(clean.fields) == {"map"}
    D, T = clean.data["map"].shape
    assert (D, T) == (900, 3000)
    sigma = 2e-4
    noise = torch.as_tensor((sigma * np.random.default_rng(21).standard_normal((D, T))).astype(np.float32)).to(DEV)
    clean.data = {"map": torch.as_tensor(clean.data["map"]).to(DEV), "noise": noise}
    glitchy = TOD({"map": clean.data["map"], "noise": noise.clone()}, clean.dets, clean.coords, units="K_RJ", metadata=dict(clean.metadata))
    onsets = flagging.inject_glitches(glitchy.data["noise"], 1, (50 * sigma, 500 * sigma), 3.0, seed=SEED)
    assert int(onsets.sum()) == D and not bool(onsets[:, 0].any()) and not bool(onsets[:, -1].any())
    flagged = glitchy.flag_glitches(ctx=gpu_ctx)
    fraction = flagged.metadata["glitches"]["flagged_fraction"]
    found = int((flagged.flags[onsets] != 0).sum())
    residual = {}
    for name, tod in (("clean", clean), ("glitchy", glitchy), ("flagged", flagged)):
        mapper = BinMapper([tod], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="I",
                           nu=[b.center for b in bands], frame="ra/dec", units="K_RJ")
        out = mapper.run()
        assert out.data.shape[-2:] == (n, n) and np.allclose(out.xi, sky.xi, atol=1e-12) and np.allclose(out.eta, sky.eta, atol=1e-12)
        m0, m1 = sky.data[0, 0], out.data[0, :]
        w = mapper.products["weight"][0, -1]
        assert (w > 0).mean() > 0.5
        residual[name] = np.sqrt(np.nansum(w * (m1 - m0) ** 2, axis=(-1, -2)) / np.nansum(w))
    print(f"onsets flagged {found} of {D}, flagged fraction {fraction:.4%}; weighted rms residual per band [K_RJ]: clean",
          residual["clean"], "glitchy", residual["glitchy"], "flagged", residual["flagged"])
    assert found == D
    assert fraction <= 0.02
    assert residual["clean"].shape == (3,)
    assert np.all(residual["flagged"] <= 1.1 * residual["clean"])
    assert np.all(residual["glitchy"] >= 3 * residual["clean"])
