"""GPU tier: mrx_tod_gram against exact integer sums and within its stated bound, its reproducibility and independence,
the C entry's refusals, and maria_amd.covariance and the TOD methods built on it against tests/covariance_ref.py."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import covariance_ref as ref
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ROW_COUNTS = (1, 31, 32, 33, 127, 129, 257)


def lengths():
    from maria_amd._lib import GRAM_BLOCK as B

    return (1, 2, 3, B - 1, B, B + 1, 2 * B + 3)  # time is not split across workgroups: there is no slice length


def padded(host, pad, offset, fill):
    """A device view [D, T] of ``host`` inside a buffer of row pitch T + pad that starts ``offset`` elements into its
    allocation, the rest of the buffer holding ``fill``."""
    import torch

    D, T = host.shape
    ld = T + pad
    buf = torch.full((D * ld + offset + 8,), fill, dtype=torch.as_tensor(host).dtype, device=DEV)
    view = buf[offset:offset + D * ld].view(D, ld)[:, :T]
    view.copy_(torch.as_tensor(host).to(DEV))
    return buf, view


def integer_case(rng, R, T, variant):
    """Device arguments of ``covariance.gram`` and the host arrays of its reference.  Every z is an integer in -3 .. 3."""
    import torch

    listed = variant in ("permuted", "out_of_range", "padded")
    D = R + 5 if listed else R
    x = rng.integers(-1, 2, (D, T)).astype(np.float32)
    model = rng.integers(-1, 2, (D, T)).astype(np.float32) if variant in ("model_center", "padded") else None
    center = rng.integers(-1, 2, D).astype(np.float64) if variant in ("model_center", "padded") else None
    flags = None
    if variant in ("flags", "padded", "permuted", "out_of_range"):
        flags = (rng.random((D, T)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (D, T)).astype(np.uint8)
    rows = None
    if listed:
        rows = rng.permutation(D)[:R].astype(np.int64)
        if variant == "out_of_range":
            rows[rng.random(R) < 0.3] = -1
            rows[0] = D if R > 1 else rows[0]
            if R > 2:
                rows[R // 2] = 2**31 - 1
    host = dict(x=x, model=model, center=center, flags=flags, rows=rows)
    xs, ms, fs = x.copy(), None if model is None else model.copy(), None if flags is None else flags.copy()
    if listed:  # rows the list does not name hold what must not be read
        unnamed = np.setdiff1d(np.arange(D), rows)
        xs[unnamed] = np.nan
        if fs is not None:
            fs[unnamed] = 255
    keep = []
    if variant == "padded":  # odd pitches, pointers 4 bytes off a 16-byte line (flags: 1 byte), sentinels past T
        b1, dx = padded(xs, 3, 1, float("nan"))
        b2, dm = padded(ms, 5, 3, float("nan"))
        b3, df = padded(fs, 7, 1, 255)
        keep = [b1, b2, b3]
    else:  # contiguous: 16-byte accesses wherever T is a multiple of 4
        dx = torch.as_tensor(xs).to(DEV)
        dm = None if ms is None else torch.as_tensor(ms).to(DEV)
        df = None if fs is None else torch.as_tensor(fs).to(DEV)
    dev = dict(x=dx, model=dm, flags=df, center=None if center is None else torch.as_tensor(center).to(DEV),
               rows=None if rows is None else torch.as_tensor(rows).to(DEV), keep=keep)
    return host, dev


@pytest.mark.parametrize("variant", ["plain", "flags", "model_center", "padded", "permuted", "out_of_range"])
def test_exact_integers_bit_for_bit(gpu_ctx, variant):
    """z in -3 .. 3: every float32 partial sum is an integer below 2^24, G is the int64 product and n the exact count, at
    every row count around the 32-row tile and the 128-row block and every length around the float32 block."""
    import torch

    from maria_amd import covariance

    rng = np.random.default_rng({"plain": 1, "flags": 2, "model_center": 3, "padded": 4, "permuted": 5, "out_of_range": 6}[variant])
    for R in ROW_COUNTS:
        for T in lengths():
            h, d = integer_case(rng, R, T, variant)
            G, n = covariance.gram(d["x"], center=d["center"], rows=d["rows"], flags=d["flags"], model=d["model"], ctx=gpu_ctx)
            torch.cuda.synchronize()
            D = h["x"].shape[0]
            z = ref.z_of(h["x"], h["model"], h["flags"], h["center"])
            want = ref.gram_exact_int(z, h["rows"])
            got = G.cpu().numpy()
            # (a sentinel that was read shows here: NaN in x past T and in the unnamed rows, 255 in their flags)
            assert got.shape == (R, R) and np.array_equal(got, want.astype(np.float64)), (variant, R, T, np.abs(got - want).max())
            assert np.array_equal(n.cpu().numpy(), ref.counts(h["flags"], D, T, h["rows"])), (variant, R, T)


def test_gaussian_data_within_the_stated_bound(gpu_ctx, capsys):
    """Gaussian data with a model, a centre and flags: per element |G - float64 sum of the same rounded z| within
    (B 2^-24 + ceil(T / B) 2^-53) sum |z_i z_j|, the header's bound.  The largest ratio seen is printed."""
    import torch

    from maria_amd import covariance
    from maria_amd._lib import GRAM_BLOCK as B

    rng = np.random.default_rng(11)
    worst = 0.0
    for R in (33, 129, 257):
        for T in lengths() + (4 * B + 17,):
            x = (3.0 * rng.standard_normal((R, T)) + 10.0).astype(np.float32)
            model = rng.standard_normal((R, T)).astype(np.float32)
            center = 10.0 + rng.standard_normal(R)
            flags = (rng.random((R, T)) < 0.1).astype(np.uint8)
            G, _ = covariance.gram(torch.as_tensor(x).to(DEV), center=torch.as_tensor(center).to(DEV), flags=torch.as_tensor(flags).to(DEV),
                                   model=torch.as_tensor(model).to(DEV), counts=False, ctx=gpu_ctx)
            want, A = ref.gram(ref.z_of(x, model, flags, center))
            err = np.abs(G.cpu().numpy() - want)
            lim = ref.bound(A, T, B)
            assert np.all(err <= lim), (R, T, float((err / np.where(lim > 0, lim, 1)).max()))
            worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0)
    with capsys.disabled():
        print(f"\nmrx_tod_gram: largest error / bound over the Gaussian cases: {worst:.3f}")
    assert 0.0 < worst <= 1.0


def test_reproducible_and_independent_of_the_rest_of_the_call(gpu_ctx):
    """The same bits on a second call; for a pair of rows alone as inside 257; with other rows added to D; at the other
    alignment; with 1e30 and NaN under the flags.  G is symmetric bit for bit, and an unflagged NaN stays in its row and
    column."""
    import torch

    from maria_amd import covariance
    from maria_amd._lib import GRAM_BLOCK as B

    rng = np.random.default_rng(5)
    R, T = 257, 2 * B + 3
    x = rng.standard_normal((R, T)).astype(np.float32)
    flags = (rng.random((R, T)) < 0.1).astype(np.uint8)
    center = 0.1 * rng.standard_normal(R)
    dx, df, dc = torch.as_tensor(x).to(DEV), torch.as_tensor(flags).to(DEV), torch.as_tensor(center).to(DEV)
    G, n = covariance.gram(dx, center=dc, flags=df, ctx=gpu_ctx)
    G2, n2 = covariance.gram(dx, center=dc, flags=df, ctx=gpu_ctx)
    bits = lambda t: t.view(torch.int64)  # noqa: E731
    assert torch.equal(bits(G), bits(G2)) and torch.equal(n, n2)
    assert torch.equal(bits(G), bits(G.T.contiguous())) and torch.equal(n, n.T)
    for i, j in ((3, 200), (256, 0), (130, 131)):
        Gp, np_ = covariance.gram(dx, center=dc, rows=np.array([i, j]), flags=df, ctx=gpu_ctx)
        assert torch.equal(bits(Gp), bits(G[[i, j]][:, [i, j]].contiguous())) and torch.equal(np_, n[[i, j]][:, [i, j]]), (i, j)
    # other rows added to D, an odd pitch and a pointer off the 16-byte line, 1e30 and NaN under the flags
    big = np.full((R + 40, T), np.nan, np.float32)
    bflags = np.full((R + 40, T), 255, np.uint8)
    where = rng.permutation(R + 40)[:R]
    big[where], bflags[where] = x, flags
    hostile = big.copy()
    put = bflags != 0
    hostile[put] = np.where(rng.random(int(put.sum())) < 0.5, np.float32(1e30), np.float32("nan"))
    bcenter = np.zeros(R + 40)
    bcenter[where] = center
    _, hx = padded(hostile, 3, 1, float("nan"))
    _, hf = padded(bflags, 5, 3, 255)
    Gh, nh = covariance.gram(hx, center=torch.as_tensor(bcenter).to(DEV), rows=where, flags=hf, ctx=gpu_ctx)
    assert torch.equal(bits(Gh), bits(G)) and torch.equal(nh, n)
    # an unflagged NaN
    xn = x.copy()
    row = 77
    t = int(np.flatnonzero(flags[row] == 0)[0])
    xn[row, t] = np.nan
    Gn, nn = covariance.gram(torch.as_tensor(xn).to(DEV), center=dc, flags=df, ctx=gpu_ctx)
    hit = torch.zeros((R, R), dtype=torch.bool, device=DEV)
    hit[row, :] = hit[:, row] = True
    assert bool(torch.isnan(Gn[hit]).all()) and torch.equal(bits(Gn[~hit]), bits(G[~hit])) and torch.equal(nn, n)


def test_counts_without_flags_and_without_counts(gpu_ctx):
    import torch

    from maria_amd import covariance

    x = torch.ones((5, 40), dtype=torch.float32, device=DEV)
    G, n = covariance.gram(x, rows=np.array([4, -1, 0]), ctx=gpu_ctx)
    want = np.array([[40, 0, 40], [0, 0, 0], [40, 0, 40]])
    assert np.array_equal(n.cpu().numpy(), want) and np.array_equal(G.cpu().numpy(), want.astype(np.float64))
    assert covariance.gram(x, counts=False, ctx=gpu_ctx)[1] is None


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T, R = 4, 300, 3
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    model = torch.zeros((D, T), dtype=torch.float32, device=DEV)
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    rows = torch.as_tensor(np.array([2, 0, 1], np.int32)).to(DEV)
    center = torch.zeros(D, dtype=torch.float64, device=DEV)
    G = torch.full((R, R), 7.0, dtype=torch.float64, device=DEV)
    n = torch.full((R, R), 12345, dtype=torch.int32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    ok = (ptr(x), T, ptr(model), T, ptr(flags), T, D, T, ptr(rows), R, ptr(center), ptr(G), ptr(n))

    def put(*pairs):
        args = list(ok)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    bad = {"null x": put((0, None)), "null G": put((11, None)), "D 0": put((6, 0)), "T 0": put((7, 0)), "R 0": put((9, 0)), "R -1": put((9, -1)),
           "ld_x < T": put((1, T - 1)), "ld_m < T": put((3, T - 1)), "ld_f < T": put((5, T - 1))}
    for name, args in bad.items():
        assert lib.mrx_tod_gram(hd, *args) == -1, name
        assert b"mrx_tod_gram" in lib.mrx_last_error(hd), name
    torch.cuda.synchronize()
    assert bool((G == 7.0).all()) and bool((n == 12345).all())
    # a pitch of an array that is not given is not looked at; rows, centre and counts may be null
    assert lib.mrx_tod_gram(hd, *put((2, None), (3, 0), (4, None), (5, 0), (8, None), (9, D - 1), (10, None), (12, None))) == 0
    torch.cuda.synchronize()
    assert bool((G == float(T)).all()) and bool((n == 12345).all())


# ---- the Python layer: covariance, remove_modes, cut_uncorrelated ---------------------------------------------------------


def fixture_tod(fields, flags=None):
    """A TOD of [96, 4096] host fields on a daisy scan: two bands of 48 positions, polarisation angle 0 (an I weight of
    exactly 1 / 2: tests/test_gpu_downsample.py)."""
    import torch

    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates
    from test_host_covariance import D_BAND, GROUPS, T_FIX

    t = 1.7e9 + np.arange(T_FIX) / 50.0
    az, el = synthetic.daisy_scan(t, radius_deg=0.3)
    bands = [Band(center=93e9, width=27e9, name="f093"), Band(center=150e9, width=41e9, name="f150")]
    offsets = np.concatenate([synthetic.hex_pack(D_BAND, np.radians(0.4))] * 2)
    dets = Detectors(offsets, bands, GROUPS.copy(), gamma=np.zeros(2 * D_BAND))
    data = {k: torch.as_tensor(v).to(DEV) for k, v in fields.items()}
    tod = TOD(data, dets, Coordinates(t, az, el, offsets=dets.offsets), units="K_RJ", metadata={"latitude": -23.0, "longitude": -67.8},
              flags=None if flags is None else torch.as_tensor(flags).to(DEV))
    return tod, float(np.degrees(az.mean())), float(np.degrees(el.mean())), bands


@pytest.fixture(scope="module")
def modes(gpu_ctx):
    from test_host_covariance import modes_fixture

    x, flags, sigma, _ = modes_fixture()
    tod, _, _, _ = fixture_tod({"signal": x}, flags)
    return dict(x=x, flags=flags, sigma=sigma, tod=tod)


def test_covariance_against_the_reference(gpu_ctx, modes):
    """cov, corr and valid of every group against the float64 sums of the same rounded z (the device's own means), the
    kernel's bound b on G carried through the quotients: cov within b / n, and corr = G_ij / sqrt(G_ii G_jj) n-factors
    apart within (b_ij + |G_ij| (b_ii / G_ii + b_jj / G_jj) / 2) / sqrt(G_ii G_jj), each plus 8 float64 roundings."""
    import torch

    from maria_amd import covariance
    from maria_amd._lib import GRAM_BLOCK as B
    from test_host_covariance import GROUPS

    x, flags = modes["x"], modes["flags"].copy()
    flags[5] = 1          # a row with nothing kept
    flags[60, 6:] = 1     # a row with fewer than min_hits kept
    flags[70, ::2] = 1    # pairs of full rows with few common samples
    dx, df = torch.as_tensor(x).to(DEV), torch.as_tensor(flags).to(DEV)
    cov = covariance.covariance(dx, groups=GROUPS, n_groups=2, flags=df, min_hits=8, ctx=gpu_ctx)
    mean = cov.mean.cpu().numpy()
    want_mean, want_hits = ref.row_means(x, None, flags)
    np.testing.assert_allclose(mean, want_mean, rtol=1e-12, atol=1e-12)
    z = ref.z_of(x, None, flags, mean)
    T = x.shape[1]
    eps = 8 * 2.0**-53
    for g, cg in enumerate(cov.groups):
        rows = np.flatnonzero(GROUPS == g)
        assert cg.rows.cpu().numpy().tolist() == rows.tolist() and np.array_equal(cg.hits.cpu().numpy(), want_hits[rows])
        G, A = ref.gram(z, rows)
        n = ref.counts(flags, x.shape[0], T, rows)
        b = ref.bound(A, T, B)
        assert np.array_equal(cg.n.cpu().numpy(), n) and np.all(np.abs(cg.G.cpu().numpy() - G) <= b)
        w_cov, w_corr, valid, unusable = ref.finish_group(G, n, 8)
        assert np.array_equal(cg.valid.cpu().numpy(), valid) and np.array_equal(cg.unusable.cpu().numpy(), unusable)
        assert unusable.sum() == 1 and not valid.all()
        assert np.all(np.abs(cg.cov.cpu().numpy() - w_cov) <= np.where(valid, b / np.maximum(n, 1), 0) + eps * np.abs(w_cov))
        dG = np.where(unusable, 1.0, np.diag(G))
        rel = np.where(unusable, 0.0, np.diag(b) / dG)
        lim = (b + np.abs(G) * (rel[:, None] + rel[None, :]) / 2) / np.sqrt(dG[:, None] * dG[None, :])
        # (corr carries n_ij / sqrt(n_ii n_jj), exact counts, on both sides)
        scale = np.sqrt(np.diag(n)[:, None] * np.diag(n)[None, :]) / np.maximum(n, 1)
        assert np.all(np.abs(cg.corr.cpu().numpy() - w_corr) <= lim * scale + eps * np.abs(w_corr))
    assert np.array_equal(cov.usable.cpu().numpy(), ~np.isin(np.arange(96), [5, 60]))
    assert float(cov.sigma[5]) == 0.0 and float(cov.sigma[0]) > 0


def test_remove_modes_against_the_reference_fed_the_devices_gram(gpu_ctx, modes):
    """TOD.remove_modes(2) on the modes fixture against tests/covariance_ref.remove_modes fed the device's own G and n, so
    that what is compared is everything after the Gram matrix, not the sensitivity of eigenvectors to it.

    The tolerance.  Device and reference take the same G and n, so their eigenvectors differ by float64 rounding
    (1e-15 over an eigenvalue gap above 3), and so do the float64 sums S, W, N, r of the existing kernels (DESIGN 3.22:
    within 2^-53 times the terms' magnitudes times the length).  What can differ visibly is a float32 rounding that
    falls the other way: a template sample B_k(t) = float32(S / W) by one unit in its last place, 2^-23 |B_k|, which moves
    a coefficient by at most that share of itself to first order; the subtracted combination f = float32(sum a_k B_k) by
    one more unit, 2^-23 |f|; and the output x - f by a float32 rounding of the result, 2^-24 |y|.  With
    c = max_t sum_k |a_k B_k(t)| of the detector: |dy| <= 2^-23 (3 c) + 2^-24 |y| + slack, asked as 4 * 2^-23 c + 2^-23 max|y|."""
    import torch

    from maria_amd import covariance
    from test_host_covariance import GROUPS, residual_ceiling, rms_over_white

    x, flags, sigma, tod = modes["x"], modes["flags"], modes["sigma"], modes["tod"]
    kept = tod.data["signal"].clone()
    out = tod.remove_modes(2, ctx=gpu_ctx)
    assert torch.equal(tod.data["signal"], kept) and "modes" not in tod.metadata and torch.equal(out.flags, tod.flags)
    assert out.dets is tod.dets and out.coords is tod.coords and out.units == tod.units
    rec = out.metadata["modes"]
    assert rec["n_modes"] == 2 and rec["n_groups"] == 2 and rec["eigenvalues"].shape == (2, 2) and rec["loadings"].shape == (96, 2)
    assert rec["coefficients"].shape == (96, 3) and rec["templates"].shape == (2, 3, 4096) and rec["failed_rows"].size == 0 and not rec["remove_mean"]
    cov = covariance.covariance(kept, groups=GROUPS, n_groups=2, flags=tod.flags, ctx=gpu_ctx)
    own = lambda g, rows, mean: (cov.groups[g].G.cpu().numpy(), cov.groups[g].n.cpu().numpy())  # noqa: E731
    y, B, a, eig, U = ref.remove_modes(x, flags, GROUPS, 2, own, 2)
    got = out.data["signal"].cpu().numpy()
    keep = flags == 0
    np.testing.assert_allclose(rec["eigenvalues"], eig, rtol=1e-10)
    np.testing.assert_allclose(rec["loadings"], U, rtol=0, atol=1e-9)
    c = np.abs(a[:, 1:, None] * B[GROUPS].astype(np.float64)[:, 1:, :]).sum(axis=1).max(axis=1)
    tol = 4 * 2.0**-23 * c + 2.0**-23 * np.abs(np.where(keep, y, 0)).max(axis=1)
    err = np.abs(np.where(keep, got.astype(np.float64) - y, 0.0)).max(axis=1)
    print(f"remove_modes(2): largest |device - reference| / tolerance {float((err / tol).max()):.3f}")
    assert np.all(err <= tol)
    # under the flags the same subtraction was made from the 1e30 that sits there
    assert np.array_equal(got[~keep], y[~keep])
    r_dev, r_ref = rms_over_white(got, flags, sigma), rms_over_white(y, flags, sigma)
    assert np.all(np.abs(r_dev - r_ref) <= 1e-5) and np.all((r_dev >= 0.93) & (r_dev <= residual_ceiling()))
    # one mode, or the common mode, leaves the second
    outer = np.tile(np.abs(np.linspace(-1, 1, 48)) > 1 / 3, 2)
    r1 = rms_over_white(tod.remove_modes(1, ctx=gpu_ctx).data["signal"].cpu().numpy(), flags, sigma)
    rc = rms_over_white(tod.remove_common_mode(ctx=gpu_ctx).data["signal"].cpu().numpy(), flags, sigma)
    assert np.all(r1[outer] > 2.0) and np.all(rc[outer] > 2.0)
    # remove_mean takes the constant too
    flat = tod.remove_modes(2, remove_mean=True, ctx=gpu_ctx).data["signal"].cpu().numpy()
    assert np.all(np.abs(np.where(keep, flat, 0).sum(axis=1) / keep.sum(axis=1)) < 1e-3)
    with pytest.raises(ValueError, match="n_modes"):
        tod.remove_modes(8, ctx=gpu_ctx)


def test_tod_covariance_record(gpu_ctx, modes):
    tod = modes["tod"]
    out, cov = tod.covariance(ctx=gpu_ctx)
    rec = out.metadata["covariance"]
    assert out.data is tod.data and "covariance" not in tod.metadata and rec["n_groups"] == 2 and len(cov.groups) == 2
    assert [g["unusable"] for g in rec["groups"]] == [0, 0] and all(0.85 < g["leading_share"] < 0.97 for g in rec["groups"])
    with pytest.raises(ValueError, match="field"):
        tod.covariance(field="nothing", ctx=gpu_ctx)


def test_cut_uncorrelated_takes_exactly_the_injected_rows(gpu_ctx):
    """The cut fixture with five rows made uncorrelated: cut_uncorrelated flags exactly those, every sample of them; TOD.cut
    on the same data flags none of them; and BinMapper of the result equals BinMapper of the clean TOD with the same
    flags bit for bit.  The samples are multiples of one grain and the I weight is 1 / 2, so the mapper's float64 sums are
    exact in whatever order its atomics add (tests/test_gpu_cuts.py)."""
    import torch

    from maria_amd import covariance
    from maria_amd.mappers import BinMapper
    from test_host_covariance import CHUNK, INJECTED, cut_fixture

    clean, _ = cut_fixture()
    grain = 2.0 ** (np.ceil(np.log2(32 * float(np.abs(clean).max()))) - 26)
    clean = (np.round(clean.astype(np.float64) / grain) * grain).astype(np.float32)
    dirty = covariance.inject_uncorrelated(clean, INJECTED)
    tod, az, el, bands = fixture_tod({"signal": dirty})
    out, verdict = tod.cut_uncorrelated(ctx=gpu_ctx)
    assert np.flatnonzero(verdict["cut"]).tolist() == INJECTED and out.metadata["uncorrelated"]["cut_detectors"].tolist() == INJECTED
    assert not verdict["unusable"].any() and not verdict["below"].any() and tod.flags is None and "uncorrelated" not in tod.metadata
    flags = out.flags.cpu().numpy()
    want = np.zeros_like(flags)
    want[INJECTED] = 1
    assert np.array_equal(flags, want) and torch.equal(out.data["signal"], tod.data["signal"])
    print("scores of the injected rows", verdict["score"][INJECTED].round(4), "thresholds", verdict["threshold"].round(4))
    by_stats = tod.cut(bounds=CHUNK, ctx=gpu_ctx).metadata["cuts"]["cut_detectors"].tolist()
    assert not set(by_stats) & set(INJECTED)
    loud, _ = tod.cut_uncorrelated(min_correlation=0.99, value=4, ctx=gpu_ctx)  # every row is below 0.99
    assert bool((loud.flags == 4).all())
    free, _, _, _ = fixture_tod({"signal": clean}, flags)
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="I", nu=[b.center for b in bands], frame="az/el", units="K_RJ")
    maps = {}
    for name, t in (("cut", out), ("free", free), ("dirty", tod)):
        mapper = BinMapper([t], **kw)
        mapper.run()
        maps[name] = np.asarray(mapper.products["data"], np.float64)
    assert np.isfinite(maps["free"]).mean() > 0.05
    assert np.array_equal(maps["cut"].view(np.int64), maps["free"].view(np.int64))
    assert not np.array_equal(maps["dirty"].view(np.int64), maps["free"].view(np.int64))
