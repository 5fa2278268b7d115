"""mrx_tod_line_normal, mrx_tod_line_apply, maria_amd.lines and TOD.remove_lines on the device, against the
numpy float64 reference of tests/lines_ref.py.

The reference's sums are math.fsum over the rounded products of its own carriers, which are correctly rounded (long
double, one rounding).  A device sum of a segment of n samples may differ from it by the worst case of any float64
summation order and fsum's half ulp, (n + 1) 2^-53 sum|terms|, and by what the carriers differ: the device library's
float64 sinpi and cospi are documented to 2 ulp, the reference adds 1, an ulp of a carrier is at most 2^-52, so
EPS_CARRIER = 3 * 2^-52 times sum|d term / d carrier| (test_host_lines.sum_bounds; what was measured is in DESIGN 3.37).
Where the carriers are exactly 0 and +-1 (1/4 and 1/2 cycle a sample) and the data small integers, every sum that does
not involve the baseline's slope u is exact in any order and is compared bit for bit.  The inputs live in
tests/test_host_lines.py, which shows on them that the mistakes these bounds are there for exceed them."""

import functools
import math

import lines_ref as ref
import numpy as np
import pytest
from test_gpu_flagging import device_rows, untouched_outside
from test_host_lines import COMBOS, EPS_CARRIER, ROWS, TIMES, generic_nu, make_bounds, quarter_nu, rows, sum_bounds

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def to_device(x, model, flags, padded):
    """Padded pitches in buffers that start one (x, flags) or three (model) elements off alignment, or plain tensors."""
    T = x.shape[1]
    pads = ((T + 3, 1), (T + 5, 3), (T + 1, 1)) if padded else ((T, 0),) * 3
    bufs = device_rows(x, *pads[0], -3.0), device_rows(model, *pads[1], -5.0), device_rows(flags, *pads[2], 9)
    return [b for b, _ in bufs], [v for _, v in bufs]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def without_slope(n_poly, K):
    """The entries of N [K, K] and r [K] that do not involve B_1 = u (present from n_poly = 2 on)."""
    keep = np.ones(K, bool)
    if n_poly == 2:
        keep[1] = False
    return keep[:, None] & keep[None, :], keep


def normal_case(gpu_ctx, D, T, n_poly, L, with_flags, with_model, padded, exact):
    import torch

    from maria_amd import lines

    K = n_poly + 2 * L
    seed = 1000 * T + 10 * D + K
    bounds = make_bounds(T, 10 * K + T)
    x, model, flags = rows(D, T, seed, exact)
    nu = quarter_nu(D, L) if exact else generic_nu(D, L, T + D)
    if T >= 64 and len(bounds) > 2:
        flags[D - 1, bounds[1]:bounds[2]] = 2  # one segment wholly flagged in the last row
    bufs, (xv, mv, fv) = to_device(x, model, flags, padded)
    before = [b.clone() for b in bufs]
    kw = dict(flags=fv if with_flags else None, model=mv if with_model else None)
    N, r, hits = lines.normal_equations(xv, bounds, nu, n_poly=n_poly, ctx=gpu_ctx, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"
    S = len(bounds) - 1
    assert N.dtype == r.dtype == torch.float64 and hits.dtype == torch.int64
    assert tuple(N.shape) == (D, S, K, K) and tuple(r.shape) == (D, S, K) and tuple(hits.shape) == (D, S)
    N_ref, r_ref, h_ref, aN, ar, dN, dr = ref.normal_equations(x, bounds, nu, n_poly, flags=flags if with_flags else None,
                                                               model=model if with_model else None)
    where = (D, T, n_poly, L, with_flags, with_model, padded)
    N_got, r_got = N.cpu().numpy(), r.cpu().numpy()
    np.testing.assert_array_equal(hits.cpu().numpy(), h_ref, err_msg=str(where))  # exact everywhere
    assert np.array_equal(N_got, N_got.transpose(0, 1, 3, 2)), where
    empty = np.diff(bounds) == 0
    assert not N_got[:, empty].any() and not r_got[:, empty].any() and not h_ref[:, empty].any()
    bN, br = sum_bounds(bounds, aN, ar, dN, dr)
    if exact:
        mN, mr = without_slope(n_poly, K)
        assert np.array_equal(bits(N_got[:, :, mN]), bits(N_ref[:, :, mN])) and np.array_equal(bits(r_got[:, :, mr]), bits(r_ref[:, :, mr])), where
        bN, br = bN - EPS_CARRIER * dN, br - EPS_CARRIER * dr  # the carriers are exact: the slope's sums within the order's bound
    assert np.all(np.abs(N_got - N_ref) <= bN) and np.all(np.abs(r_got - r_ref) <= br), where
    if exact and with_flags:  # what a flagged sample holds changes no bit; a second call neither
        for fill in (None, 1e30, float("nan")):
            if fill is not None:
                xv[fv != 0] = fill
            again = lines.normal_equations(xv, bounds, nu, n_poly=n_poly, ctx=gpu_ctx, **kw)
            assert torch.equal(again[0], N) and torch.equal(again[1], r) and torch.equal(again[2], hits), (where, fill)
    return float(max((np.abs(r_got - r_ref) / np.where(br > 0, br, 1)).max(), (np.abs(N_got - N_ref) / np.where(bN > 0, bN, 1)).max()))


@pytest.mark.parametrize("n_poly,L", COMBOS)
def test_small_integers_at_quarter_cycles_bit_for_bit(gpu_ctx, n_poly, L):
    """nu of 1/4 and 1/2 cycle a sample: the carriers are exactly 0 and +-1, every product with small-integer data an
    integer, every sum exact in any order: hits exact, N and r bit for bit (the sums with the slope u within the bound of
    the order alone), with 1e30 and NaN under the flags, and on a second call."""
    for i, T in enumerate(TIMES):
        D = ROWS[(i + n_poly + L) % 3]
        normal_case(gpu_ctx, D, T, n_poly, L, with_flags=True, with_model=i % 2 == 0, padded=i % 2 == 1, exact=True)
        if T in (2, 257, 1025):
            normal_case(gpu_ctx, ROWS[(i + n_poly + L + 1) % 3], T, n_poly, L, with_flags=False, with_model=True, padded=i % 2 == 0, exact=True)


@pytest.mark.parametrize("n_poly,L", COMBOS)
def test_sums_within_the_bound(gpu_ctx, n_poly, L):
    """Gaussian rows, generic frequencies, flags at 30 % (with a segment wholly flagged) and at 0, a model, padded pitches."""
    worst = 0.0
    for i, T in enumerate(TIMES):
        D = ROWS[(i + n_poly + L) % 3]
        worst = max(worst, normal_case(gpu_ctx, D, T, n_poly, L, with_flags=True, with_model=True, padded=(i + L) % 2 == 0, exact=False))
        if T in (1, 65, 1023):
            worst = max(worst, normal_case(gpu_ctx, ROWS[(i + n_poly + L + 1) % 3], T, n_poly, L, with_flags=False, with_model=False,
                                           padded=(i + L) % 2 == 1, exact=False))
    print(f"n_poly {n_poly}, L {L}: max |sum - ref| / bound = {worst:.3g}")


def carriers_on_device(gpu_ctx, nu, t0, n):
    """(cos, sin) [D, L, n] float64 as the kernel evaluates them at the samples t0 .. t0 + n - 1: r of n one-sample
    segments of a row of ones with n_poly = 0 is the carrier times 1.0."""
    import torch

    from maria_amd import lines

    D = nu.shape[0]
    x = torch.ones((D, t0 + n), dtype=torch.float32, device=DEV)
    _, r, hits = lines.normal_equations(x, np.arange(t0, t0 + n + 1, dtype=np.int32), nu, n_poly=0, ctx=gpu_ctx)
    assert bool((hits == 1).all())
    r = r.cpu().numpy()  # [D, n, 2 L]
    return r[:, :, 0::2].transpose(0, 2, 1), r[:, :, 1::2].transpose(0, 2, 1)


def test_the_carriers_against_the_reference(gpu_ctx):
    """Every carrier the kernel evaluates, read back through one-sample segments, within EPS_CARRIER of the reference's
    (long double, rounded once); the largest difference is printed in units of 2^-53."""
    nu = generic_nu(65, 3, 11)
    c, s = carriers_on_device(gpu_ctx, nu, 0, 4097)
    c_ref, s_ref = ref.carriers(nu, np.arange(4097))
    worst = max(np.abs(c - c_ref).max(), np.abs(s - s_ref).max())
    print(f"max |carrier - ref| = {worst / 2.0**-53:.2f} x 2^-53 over {c.size * 2} values (long double reference: {ref.HAS_LONG})")
    assert worst <= EPS_CARRIER
    assert c[:, :, 0].tolist() == [[1.0] * 3] * 65 and s[:, :, 0].tolist() == [[0.0] * 3] * 65
    # quarter cycles: exactly 0 and +-1
    c, s = carriers_on_device(gpu_ctx, np.array([[0.25, 0.5, 0.125]]), 0, 16)
    assert c[0, 0].tolist() == [1.0, 0.0, -1.0, 0.0] * 4 and s[0, 0].tolist() == [0.0, 1.0, 0.0, -1.0] * 4
    assert c[0, 1].tolist() == [1.0, -1.0] * 8 and not s[0, 1].any()
    assert c[0, 2, ::2].tolist() == [1.0, 0.0, -1.0, 0.0] * 2 and s[0, 2, ::2].tolist() == [0.0, 1.0, 0.0, -1.0] * 2


def test_phase_coherence_at_the_end_of_a_long_row(gpu_ctx):
    """nu t at t up to 2^21 - 1 with nu near 1/2: theta is one rounding of the product (<= 2^-53 theta = 1.2e-10 cycles)
    and its reduction is exact, in the kernel as in the reference, so the carriers agree within EPS_CARRIER.  One ulp of
    theta there, 2^-32 cycles, would move a carrier by 2 pi 2^-32 = 1.5e-9: two million times the bound."""
    T = 2**21
    nu = np.array([[0.5 - 2.0**-30, 0.49999, 0.4375 + 2.0**-40], [0.5, 1.0 / 3.0, 0.123456789]])
    n = 67
    c, s = carriers_on_device(gpu_ctx, nu, T - n, n)
    t = np.arange(T - n, T)
    c_ref, s_ref = ref.carriers(nu, t)
    worst = max(np.abs(c - c_ref).max(), np.abs(s - s_ref).max())
    print(f"max |carrier - ref| at t = 2^21 - {n} .. 2^21 - 1: {worst / 2.0**-53:.2f} x 2^-53")
    assert worst <= EPS_CARRIER
    assert c[1, 0].tolist() == [(-1.0) ** int(k) for k in t] and not s[1, 0].any()
    wrong = ref.sincospi(2.0 * (np.nextafter(nu[0, 0] * t, np.inf) - np.rint(nu[0, 0] * t)))
    assert max(np.abs(wrong[0] - s_ref[0, 0]).max(), np.abs(wrong[1] - c_ref[0, 0]).max()) > 1e6 * EPS_CARRIER  # what an ulp of theta would do


def test_sums_are_reproducible_alone_and_at_either_alignment(gpu_ctx):
    """The same bits on a second call, for a row alone (so also when rows are added), for a segment alone (its own two
    bounds) and at either alignment: the order is a function of the segment's ends alone."""
    import torch

    from maria_amd import lines

    D, T = 33, 4097
    x, model, flags = rows(D, T, 8, exact=False)
    dx, dm, df = (torch.as_tensor(a).to(DEV) for a in (x, model, flags))
    for n_poly, L in ((0, 1), (2, 2), (2, 3)):
        nu = generic_nu(D, L, 3)
        bounds = make_bounds(T, n_poly + L)
        S = len(bounds) - 1
        kw = dict(n_poly=n_poly, ctx=gpu_ctx)
        first = lines.normal_equations(dx, bounds, nu, flags=df, model=dm, **kw)
        again = lines.normal_equations(dx, bounds, nu, flags=df, model=dm, **kw)
        for a, c in zip(first, again):
            assert torch.equal(a, c)
        for row in (0, 16, 32):
            alone = lines.normal_equations(dx[row:row + 1], bounds, nu[row:row + 1], flags=df[row:row + 1], model=dm[row:row + 1], **kw)
            for a, c in zip(first, alone):
                assert torch.equal(a[row:row + 1], c), (n_poly, L, row)
        for s in range(S):
            alone = lines.normal_equations(dx, bounds[s:s + 2], nu, flags=df, model=dm, **kw)
            for a, c in zip(first, alone):
                assert torch.equal(a[:, s:s + 1], c), (n_poly, L, s)
        wide = [device_rows(v, 4100, 0, 0)[1] for v in (x, model, flags)]
        odd = [device_rows(v, 4101, 1, 0)[1] for v in (x, model, flags)]
        for layout in (wide, odd):
            got = lines.normal_equations(layout[0], bounds, nu, flags=layout[2], model=layout[1], **kw)
            for a, c in zip(first, got):
                assert torch.equal(a, c), (n_poly, L)


def test_a_nan_stays_where_it_is(gpu_ctx):
    """An unflagged NaN makes the r of its own (row, segment) NaN and nothing else; a non-finite frequency (through the
    C entry: the Python side refuses it) spoils its own row only."""
    import torch

    from maria_amd import lines
    from maria_amd._lib import ptr

    D, T, n_poly, L = 5, 1025, 2, 2
    K = n_poly + 2 * L
    x, model, flags = rows(D, T, 4, exact=False)
    nu = generic_nu(D, L, 9)
    bounds = make_bounds(T, 2)
    S = len(bounds) - 1
    s_bad = int(np.argmax(np.diff(bounds)))
    t_bad = int(bounds[s_bad]) + 7
    flags[2, t_bad] = 0
    dx, df = torch.as_tensor(x).to(DEV), torch.as_tensor(flags).to(DEV)
    clean = lines.normal_equations(dx, bounds, nu, n_poly=n_poly, flags=df, ctx=gpu_ctx)
    dx[2, t_bad] = float("nan")
    N, r, hits = lines.normal_equations(dx, bounds, nu, n_poly=n_poly, flags=df, ctx=gpu_ctx)
    assert torch.equal(N, clean[0]) and torch.equal(hits, clean[2]) and bool(torch.isnan(r[2, s_bad]).all())
    r[2, s_bad] = clean[1][2, s_bad]
    assert torch.equal(r, clean[1])
    dx[2, t_bad] = float(x[2, t_bad])
    bad = nu.copy()
    bad[3, 1] = np.nan
    bad[1, 0] = np.inf
    d_nu, d_bound = torch.as_tensor(bad).to(DEV), torch.as_tensor(bounds).to(DEV)
    N = torch.empty((D, S, K, K), dtype=torch.float64, device=DEV)
    r = torch.empty((D, S, K), dtype=torch.float64, device=DEV)
    gpu_ctx.call("mrx_tod_line_normal", ptr(dx), T, None, 0, ptr(df), T, D, T, ptr(d_bound), S, ptr(d_nu), L, n_poly, ptr(N), ptr(r), None)
    torch.cuda.synchronize()
    good = [0, 2, 4]
    assert torch.equal(N[good], clean[0][good]) and torch.equal(r[good], clean[1][good])
    full = torch.as_tensor(np.diff(bounds) > 8).to(DEV)
    assert bool(torch.isnan(r[3][:, n_poly + 2:][full]).all()) and torch.equal(r[3][:, :n_poly + 2], clean[1][3][:, :n_poly + 2])
    assert bool(torch.isnan(r[1][:, n_poly:n_poly + 2][full]).all()) and torch.equal(r[1][:, n_poly + 2:], clean[1][1][:, n_poly + 2:])


@pytest.mark.parametrize("n_poly,L", [(0, 1), (1, 2), (2, 3)])
def test_application_bit_for_bit_with_dyadic_coefficients(gpu_ctx, n_poly, L):
    """Carriers of 0 and +-1 and coefficients k / 8: every product and every partial sum is exact, so the float64 sum is
    the reference's in any evaluation and y its one float32 operation: bit for bit, both signs, in and out of place."""
    import torch

    from maria_amd import lines

    K = n_poly + 2 * L
    for i, T in enumerate(TIMES):
        D = ROWS[(i + K) % 3]
        rng = np.random.default_rng(T + D + K)
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        bounds = make_bounds(T, 10 * K + T)
        S = len(bounds) - 1
        nu = quarter_nu(D, L)
        a = rng.integers(-64, 65, (D, S, K)) / 8.0
        da = torch.as_tensor(a).to(DEV)
        covered = ref.covered(bounds, T)
        assert T < 3 or not covered[[0, -1]].any()
        for pitch, offset in ((T + (-T) % 4, 0), (T, 0), (T + 3, 1)):
            for sign in (-1, 1):
                want = ref.apply(x, bounds, nu, a, n_poly, sign=sign)
                assert np.array_equal(want[:, ~covered], x[:, ~covered])
                xbuf, xv = device_rows(x, pitch, offset, -3.0)
                before = xbuf.clone()
                ybuf, yv = device_rows(np.zeros_like(x), pitch + 4, offset, 7.0)
                yv.fill_(7.0)
                out = lines.apply(xv, bounds, nu, da, n_poly, sign=sign, out=yv, ctx=gpu_ctx)
                torch.cuda.synchronize()
                assert out is yv and torch.equal(xbuf, before), "the input changed"
                assert np.array_equal(bits(yv.cpu().numpy()), bits(want)), (T, D, pitch, offset, sign)
                assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"
                out = lines.apply(xv, bounds, nu, da, n_poly, sign=sign, out=xv, ctx=gpu_ctx)  # in place
                torch.cuda.synchronize()
                assert out is xv and np.array_equal(bits(xv.cpu().numpy()), bits(want)), (T, D, pitch, offset, sign, "in place")
                assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"
        dx = torch.as_tensor(x).to(DEV)
        assert np.array_equal(lines.apply(dx, bounds, nu, da, n_poly, ctx=gpu_ctx).cpu().numpy(), ref.apply(x, bounds, nu, a, n_poly, sign=-1))


@pytest.mark.parametrize("n_poly,L", COMBOS)
def test_application_within_one_float32_rounding(gpu_ctx, n_poly, L):
    """Generic frequencies and coefficients: y against x + sign * s with the reference's float64 s: the rounding of s to
    float32 and of the sum, 2^-24 (|s| + |y|), and the carriers' EPS_CARRIER sum|a| (far below them)."""
    import torch

    from maria_amd import lines

    K = n_poly + 2 * L
    for i, T in enumerate(TIMES):
        D = ROWS[(i + K) % 3]
        rng = np.random.default_rng(T + D + K)
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        bounds = make_bounds(T, 10 * K + T)
        S = len(bounds) - 1
        nu = generic_nu(D, L, T + K)
        a = rng.standard_normal((D, S, K))
        sign = 1 if i % 2 else -1
        s = ref.fit_values(bounds, nu, a, n_poly, T)
        size = np.zeros((D, T))
        for k, (lo, hi) in enumerate(ref.segments(bounds, T)):
            size[:, lo:hi] = np.abs(a[:, k, n_poly:]).sum(axis=1)[:, None]
        exact = x.astype(np.float64) + sign * s
        tol = 2.0**-24 * (np.abs(s) + np.abs(exact)) * (1 + 1e-6) + 2 * EPS_CARRIER * size
        _, xv = device_rows(x, T + 3, 1, -3.0)
        got = lines.apply(xv, bounds, nu, torch.as_tensor(a).to(DEV), n_poly, sign=sign, ctx=gpu_ctx).cpu().numpy()
        covered = ref.covered(bounds, T)
        assert np.array_equal(got[:, ~covered], x[:, ~covered])
        assert np.all(np.abs(got.astype(np.float64) - exact) <= tol), (T, D, n_poly, L)


def test_inject_lines(gpu_ctx):
    """Four lines (two calls of three at the most), [L] and [D, L] arguments, out of place and in place."""
    import torch

    from maria_amd import lines

    D, T, fs = 3, 2000, 100.0
    rng = np.random.default_rng(12)
    x = rng.standard_normal((D, T)).astype(np.float32)
    freqs, amps = np.array([3.3, 7.25, 12.5, 41.0]), np.array([1.0, 0.5, 2.0, 0.25])
    phases = rng.uniform(-3, 3, (D, 4))
    t = np.arange(T) / fs
    want = x + sum(amps[l] * np.cos(2 * np.pi * freqs[l] * t[None, :] + phases[:, l, None]) for l in range(4))
    dx = torch.as_tensor(x).to(DEV)
    y = lines.inject_lines(dx, freqs, amps, phases, fs, ctx=gpu_ctx)
    assert y is not dx and torch.equal(dx, torch.as_tensor(x).to(DEV))
    assert np.abs(y.cpu().numpy() - want).max() < 4 * 2.0**-23 * np.abs(want).max()
    z = lines.inject_lines(dx, freqs, amps, phases, fs, out=dx, ctx=gpu_ctx)
    assert z is dx and torch.equal(z, y)


def test_hostile_bounds_are_clamped(gpu_ctx):
    """The C entries with bounds below 0, above T and reversed: clamped, a reversed pair empty, nothing out of range."""
    import torch

    from maria_amd import lines
    from maria_amd._lib import ptr

    D, T, n_poly, L = 3, 300, 2, 1
    K = n_poly + 2 * L
    x, model, flags = rows(D, T, 21, exact=False)
    nu = generic_nu(D, L, 2)
    bufs, (xv, mv, fv) = to_device(x, model, flags, True)
    before = [b.clone() for b in bufs]
    raw = np.array([-2**31, -7, 5, 3, 3, 140, 120, T + 9, 2**31 - 1], np.int32)  # [0, 0) [0, 5) [5, 3) [3, 3) [3, 140) [140, 120) [120, 300) [300, 300)
    S = len(raw) - 1
    assert [hi - lo for lo, hi in ref.segments(raw, T)] == [0, 5, -2, 0, 137, -20, 180, 0]
    d_raw, d_nu = torch.as_tensor(raw).to(DEV), torch.as_tensor(nu).to(DEV)
    N = torch.full((D, S, K, K), 7.0, dtype=torch.float64, device=DEV)
    r = torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV)
    hits = torch.full((D, S), 12345, dtype=torch.int32, device=DEV)
    gpu_ctx.call("mrx_tod_line_normal", ptr(xv), T + 3, ptr(mv), T + 5, ptr(fv), T + 1, D, T, ptr(d_raw), S, ptr(d_nu), L, n_poly, ptr(N), ptr(r),
                 ptr(hits))
    torch.cuda.synchronize()
    N_ref, r_ref, h_ref, aN, ar, dN, dr = ref.normal_equations(x, raw, nu, n_poly, flags=flags, model=model)
    assert np.array_equal(hits.cpu().numpy(), h_ref) and h_ref[:, [0, 2, 3, 5, 7]].sum() == 0 and h_ref[:, [1, 4, 6]].all()
    assert np.all(np.abs(N.cpu().numpy() - N_ref) <= 301 * 2.0**-53 * aN + EPS_CARRIER * dN)
    assert np.all(np.abs(r.cpu().numpy() - r_ref) <= 301 * 2.0**-53 * ar + EPS_CARRIER * dr)
    # the application through the Python side, whose bounds ascend: clamped at both ends, every sample covered
    asc = np.array([-7, 5, 5, 140, T + 9], np.int32)
    a = np.random.default_rng(22).integers(-16, 17, (D, 4, K)) / 4.0
    qnu = quarter_nu(D, L)
    want = ref.apply(x, asc, qnu, a, n_poly, sign=+1)
    ybuf, yv = device_rows(np.zeros_like(x), T + 7, 1, 7.0)
    lines.apply(xv, asc, qnu, torch.as_tensor(a).to(DEV), n_poly, sign=+1, out=yv, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert np.array_equal(bits(yv.cpu().numpy()), bits(want)) and not np.array_equal(want, x)
    assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"
    # reversed bounds in the application: whichever segment a sample is given to, nothing is written outside the rows
    ybuf, yv = device_rows(np.zeros_like(x), T + 7, 1, 7.0)
    a8 = torch.zeros((D, S, K), dtype=torch.float64, device=DEV)
    gpu_ctx.call("mrx_tod_line_apply", ptr(xv), T + 3, D, T, ptr(d_raw), S, ptr(d_nu), L, n_poly, ptr(a8), -1, ptr(yv), T + 7)
    torch.cuda.synchronize()
    assert np.array_equal(yv.cpu().numpy(), x) and untouched_outside(ybuf, yv, 7.0)  # a = 0: a copy
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T, S, L, n_poly = 4, 3000, 3, 1, 1
    K = n_poly + 2 * L
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    model = torch.zeros((D, T), dtype=torch.float32, device=DEV)
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    bound = torch.as_tensor(np.array([0, 1000, 1000, T], np.int32)).to(DEV)
    nu = torch.full((D, L), 0.25, dtype=torch.float64, device=DEV)
    a = torch.ones((D, S, K), dtype=torch.float64, device=DEV)
    N = torch.full((D, S, K, K), 7.0, dtype=torch.float64, device=DEV)
    r = torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV)
    hits = torch.full((D, S), 12345, dtype=torch.int32, device=DEV)
    y = torch.full((D, T + 4), 7.0, dtype=torch.float32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    ne = (ptr(x), T, ptr(model), T, ptr(flags), T, D, T, ptr(bound), S, ptr(nu), L, n_poly, ptr(N), ptr(r), ptr(hits))
    ap = (ptr(x), T, D, T, ptr(bound), S, ptr(nu), L, n_poly, ptr(a), -1, ptr(y), T + 4)

    def put(args, *pairs):
        args = list(args)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    cases = {
        "mrx_tod_line_normal": {
            "null x": put(ne, (0, None)), "null bound": put(ne, (8, None)), "null nu": put(ne, (10, None)), "null N": put(ne, (13, None)),
            "null r": put(ne, (14, None)), "D 0": put(ne, (6, 0)), "T 0": put(ne, (7, 0)), "S 0": put(ne, (9, 0)), "S -1": put(ne, (9, -1)),
            "L 0": put(ne, (11, 0)), "L 4": put(ne, (11, 4)), "n_poly -1": put(ne, (12, -1)), "n_poly 3": put(ne, (12, 3)),
            "ld_x < T": put(ne, (1, T - 1)), "ld_m < T": put(ne, (3, T - 1)), "ld_f < T": put(ne, (5, T - 1)),
        },
        "mrx_tod_line_apply": {
            "null x": put(ap, (0, None)), "null bound": put(ap, (4, None)), "null nu": put(ap, (6, None)), "null a": put(ap, (9, None)),
            "null y": put(ap, (11, None)), "D 0": put(ap, (2, 0)), "T 0": put(ap, (3, 0)), "S 0": put(ap, (5, 0)), "L 0": put(ap, (7, 0)),
            "L 4": put(ap, (7, 4)), "n_poly -1": put(ap, (8, -1)), "n_poly 3": put(ap, (8, 3)), "sign 0": put(ap, (10, 0)),
            "sign 2": put(ap, (10, 2)), "ld_x < T": put(ap, (1, T - 1)), "ld_y < T": put(ap, (12, T - 1)),
            "in place at another pitch": put(ap, (11, ptr(x)), (12, T + 4)),
        },
    }
    for entry, bad in cases.items():
        for name, args in bad.items():
            assert getattr(lib, entry)(hd, *args) == -1, (entry, name)
            assert entry.encode() in lib.mrx_last_error(hd), (entry, name)
    torch.cuda.synchronize()
    for out in (N, r, y):
        assert bool((out == 7.0).all())
    assert bool((hits == 12345).all()) and bool((x == 1.0).all())
    # a pitch of an array that is not given is not looked at; hits may be null
    assert lib.mrx_tod_line_normal(hd, *put(ne, (2, None), (3, 0), (4, None), (5, 0), (15, None))) == 0
    torch.cuda.synchronize()
    assert N[:, :, 0, 0].tolist() == [[1000.0, 0.0, 2000.0]] * D and r[:, :, 0].tolist() == [[1000.0, 0.0, 2000.0]] * D and bool((hits == 12345).all())
    assert N[:, :, 1, 1].tolist() == [[500.0, 0.0, 1000.0]] * D and N[:, :, 2, 2].tolist() == [[500.0, 0.0, 1000.0]] * D  # cos^2 and sin^2 at 1/4
    assert lib.mrx_tod_line_normal(hd, *ne) == 0 and lib.mrx_tod_line_apply(hd, *ap) == 0
    torch.cuda.synchronize()
    assert hits.tolist() == [[1000, 0, 2000]] * D and not bool(N[:, 1].any())
    # y = 1 - (cos + sin)(2 pi t / 4): the baseline's coefficient is not applied
    assert y[:, :4].tolist() == [[0.0, 0.0, 2.0, 2.0]] * D and bool((y[:, T:] == 7.0).all())


def test_line_normal_past_the_first_trip(gpu_ctx):
    """More (row, segment) pairs than the resident grid holds (test_gpu_resident_trips.py's shape: some workgroups make
    three trips): the whole output equals the one-trip calls' in every bit, a second call too, and the rows that the
    first and the last workgroup touch are within the bound of the reference."""
    import torch
    from test_gpu_resident_trips import WAVES, on_device, place, three_ways, wave_rows, wave_shape

    from maria_amd._lib import ptr

    n_cu, R, D, S, T, bounds, n_groups = wave_shape(gpu_ctx)
    n_poly, L = 1, 1
    K = n_poly + 2 * L
    x, model, flags = rows(D, T, D, exact=False, flagged=0.1)
    flags[D - 1, bounds[2]:bounds[3]] = 2
    nu = generic_nu(D, L, D)
    (xbuf, xv, ld_x), (mbuf, mv, ld_m), (fbuf, fv, ld_f) = place(x, "odd", -3.0), place(model, "odd", -5.0), place(flags, "odd", 9)
    before = [v.clone() for v in (xbuf, mbuf, fbuf)]
    d_bound, d_nu = on_device(bounds), on_device(nu)

    def fresh():
        outs = (torch.full((D, S, K, K), 7.0, dtype=torch.float64, device=DEV), torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV),
                torch.full((D, S), 12345, dtype=torch.int32, device=DEV))
        return [(o, o) for o in outs]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_line_normal", ptr(xv[lo:hi]), ld_x, ptr(mv[lo:hi]), ld_m, ptr(fv[lo:hi]), ld_f, hi - lo, T, ptr(d_bound), S,
                     ptr(d_nu[lo:hi]), L, n_poly, ptr(outs[0][lo:hi]), ptr(outs[1][lo:hi]), ptr(outs[2][lo:hi]))

    (N, _), (r, _), (hits, _) = three_ways(launch, fresh, D, max(1, WAVES * n_cu // S))
    assert all(torch.equal(a, c) for a, c in zip((xbuf, mbuf, fbuf), before)), "an input changed"
    sub = wave_rows(D, S, n_groups, R)
    sub = sub[:: max(1, sub.size // 40)]  # the loop reference on some forty of them, the first and those of the last trips included
    N_ref, r_ref, h_ref, aN, ar, dN, dr = ref.normal_equations(x[sub], bounds, nu[sub], n_poly, flags=flags[sub], model=model[sub])
    assert np.array_equal(hits.cpu().numpy()[sub], h_ref)
    bN, br = sum_bounds(bounds, aN, ar, dN, dr)
    assert np.all(np.abs(N.cpu().numpy()[sub] - N_ref) <= bN) and np.all(np.abs(r.cpu().numpy()[sub] - r_ref) <= br)


# ---- TOD.remove_lines ----

def make_tod(fields, fs=ref.FS, flags=None, band_index=None, t0=0.0):
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    D, T = next(iter(fields.values())).shape
    bands = [Band(center=93e9, width=27e9, name="f093"), Band(center=150e9, width=30e9, name="f150")]
    dets = Detectors(np.zeros((D, 2)), bands, np.zeros(D, int) if band_index is None else np.asarray(band_index, int))
    return TOD(dict(fields), dets, Coordinates(t0 + np.arange(T) / fs, np.zeros(T), np.full(T, 1.0)), units="K_RJ", flags=flags)


def rms(a):
    return math.sqrt(float((np.asarray(a, np.float64) ** 2).mean()))


@functools.lru_cache(maxsize=None)
def science_reference(per_detector=True):
    x, clean, hz, injected = ref.science_case()
    return ref.remove_lines(x, x, ref.FS, nperseg=2048, per_detector=per_detector)


@pytest.mark.parametrize("per_detector", [True, False])
def test_the_science_fixture_against_the_reference_pipeline(gpu_ctx, per_detector):
    """D = 12, T = 24 000 at 100 Hz, lines of 0.5 and 0.3 sigma at 7.3137 and 21.947 Hz whose frequency differs by 1e-4
    between the rows, on white noise and a random walk (lines_ref.science_case).  Against the float64 host pipeline of
    lines_ref.remove_lines on the same input: the same line set, the refined frequencies within 1e-9 relative, every
    sample within 2^-22 max(max|x|, max|fit|) of its row (one float32 rounding of the fit and one of the difference, the
    two fits differing by float64 roundings).  The residual, cleaned less line-free over the injected rms, is at most
    1.5 x the floor sigma sqrt(2 L S / T) / injected rms of a fit of 2 L amplitudes a chunk."""
    import torch

    x, clean, hz, injected = ref.science_case()
    D, T = x.shape
    tod = make_tod({"signal": torch.as_tensor(x.copy()).to(DEV)})
    assert abs(tod._sample_rate() / ref.FS - 1) < 1e-12
    out = tod.remove_lines(per_detector=per_detector, ctx=gpu_ctx)
    assert torch.equal(tod.data["signal"], torch.as_tensor(x.copy()).to(DEV)) and "lines" not in tod.metadata and out.flags is None
    assert out.dets is tod.dets and out.coords is tod.coords and out.units == tod.units
    y_ref, rec = science_reference(per_detector)
    meta = out.metadata["lines"]
    assert len(meta["lines"]) == 1 and meta["lines"][0].size == 2 == rec["lines"][0].size
    assert np.abs(meta["lines"][0] / rec["lines"][0] - 1).max() < 1e-4  # the spectra are float32 here, float64 there
    assert meta["nperseg"] == 2048 and meta["bounds"].tolist() == ref.chunk_bounds(T, 2048).tolist() and meta["unfitted"] == 0 == rec["unfitted"]
    assert meta["n_poly"] == 2 and meta["n_refine"] == 2 and meta["per_detector"] is per_detector and meta["into"] == "signal"
    rel = np.abs(meta["refined"] / rec["refined"] - 1).max()
    true = np.abs(meta["refined"] - hz).max()
    got = out.data["signal"].cpu().numpy()
    fit = x.astype(np.float64) - y_ref
    scale = np.maximum(np.abs(x).max(axis=1), np.abs(fit).max(axis=1))
    err = (np.abs(got.astype(np.float64) - y_ref).max(axis=1) / (2.0**-22 * scale)).max()
    floor = ref.noise_floor(2, meta["bounds"], T, 1.0, injected)
    resid = rms(got.astype(np.float64) - clean) / injected
    print(f"per_detector {per_detector}: max |refined / ref - 1| = {rel:.2e}; max |refined - true| = {true:.2e} Hz; "
          f"max |y - ref| / (2^-22 scale) = {err:.3f}; residual {resid:.4f} = {resid / floor:.3f} x the floor {floor:.4f}")
    assert rel <= 1e-9
    assert err <= 1.0
    assert resid <= 1.5 * floor
    assert np.allclose(meta["amplitude"], rec["amplitude"], rtol=1e-6) and meta["phase"].shape == (D, 12, 2)
    step = meta["refined"] - meta["found"]
    assert np.all(step == step[:1]) != per_detector  # one correction for the group, or one a detector
    assert true <= (7e-4 if per_detector else 1e-2)  # one frequency a group: the injected scatter, 2.2e-3 Hz rms at 21.9 Hz, stays


def test_a_tod_without_lines_comes_back_in_every_bit(gpu_ctx):
    import torch

    _, clean, _, _ = ref.science_case()
    flags = torch.as_tensor((np.random.default_rng(1).random(clean.shape) < 0.01).astype(np.uint8)).to(DEV)
    tod = make_tod({"noise": torch.as_tensor(clean.copy()).to(DEV), "extra": np.zeros_like(clean)}, flags=flags)
    out = tod.remove_lines(ctx=gpu_ctx)
    assert torch.equal(out.data["noise"], tod.data["noise"]) and not bool(out.data["extra"].any()) and out.data["noise"] is not tod.data["noise"]
    meta = out.metadata["lines"]
    assert [v.size for v in meta["lines"]] == [0] and meta["found"].shape == (12, 0) and meta["amplitude"].shape == (12, 12, 0) and meta["unfitted"] == 0
    assert torch.equal(out.flags, flags)


def test_given_lines_a_model_another_field_and_two_sets_of_lines(gpu_ctx):
    """``lines=`` of four frequencies (two sets: three neighbours, then one on the signal the first set is gone from),
    ``model=`` and ``into=`` a second field, two bands, flags at 5 % carried over unchanged: against the host pipeline."""
    import torch

    from maria_amd import lines

    D, T, fs = 6, 12000, ref.FS
    rng = np.random.default_rng(31)
    sky = (0.5 * np.sin(2 * np.pi * np.arange(T) / 3000.0)[None, :] * rng.uniform(0.5, 1.5, (D, 1))).astype(np.float32)
    noise = rng.standard_normal((D, T)).astype(np.float32)
    hz = np.array([31.4, 5.5, 17.25, 9.125])
    amps, phases = np.array([0.4, 1.0, 0.5, 0.7]), rng.uniform(-3, 3, (D, 4))
    dirty = lines.inject_lines(torch.as_tensor(noise).to(DEV), hz, amps, phases, fs, ctx=gpu_ctx)
    flags = (rng.random((D, T)) < 0.05).astype(np.uint8) * 2
    tod = make_tod({"map": sky, "noise": dirty}, flags=torch.as_tensor(flags).to(DEV), band_index=[0, 1] * 3)
    out = tod.remove_lines(lines=hz, chunk=10.0, n_poly=1, model=sky, into="noise", ctx=gpu_ctx)
    signal = (sky + dirty.cpu().numpy()).astype(np.float32)  # field_sum: the first field, the second added
    y_ref, rec = ref.remove_lines(signal, dirty.cpu().numpy(), fs, lines=hz, chunk=10.0, n_poly=1, groups=[0, 1] * 3, flags=flags, model=sky,
                                  nperseg=1024)
    meta = out.metadata["lines"]
    assert meta["chunk"] == 10.0 and meta["bounds"].tolist() == ref.chunk_bounds(T, 1000).tolist() and meta["into"] == "noise"
    assert np.array_equal(meta["found"], np.broadcast_to(hz, (D, 4))) and meta["unfitted"] == 0 == rec["unfitted"]
    assert np.abs(meta["refined"] / rec["refined"] - 1).max() <= 1e-9
    assert np.abs(meta["refined"] - hz).max() < 5e-3
    assert torch.equal(out.data["map"].cpu(), torch.as_tensor(sky)) and torch.equal(out.flags, tod.flags)
    got = out.data["noise"].cpu().numpy()
    scale = np.maximum(np.abs(noise).max(axis=1), amps.sum())
    err = (np.abs(got.astype(np.float64) - y_ref).max(axis=1) / (2 * 2.0**-22 * scale)).max()  # two subtractions, one a set
    print(f"max |y - ref| / (2^-21 scale) = {err:.3f}; residual rms {rms(got - noise):.4f} of injected {rms(dirty.cpu().numpy() - noise):.4f}")
    assert err <= 1.0
    assert rms(got - noise) < 0.15 * rms(dirty.cpu().numpy() - noise)
    # [D, L] frequencies, one row's own
    per_row = np.broadcast_to(hz[:2], (D, 2)).copy()
    per_row[3, 0] += 0.002
    own = tod.remove_lines(lines=per_row, chunk=10.0, model=sky, into="noise", ctx=gpu_ctx).metadata["lines"]
    assert np.array_equal(own["found"], per_row) and np.abs(own["refined"] - hz[:2]).max() < 5e-3
    for bad in (np.zeros(2), [60.0], np.zeros((D + 1, 2)) + 5.0, [np.nan]):
        with pytest.raises(ValueError, match="lines"):
            tod.remove_lines(lines=bad, ctx=gpu_ctx)


def test_after_flag_glitches_and_on_a_downsampled_tod(gpu_ctx):
    """The method in its place in the chain: behind ``flag_glitches`` (the glitches stay out of the fits, the flags are
    carried over) and on a TOD reduced by 2 (the finder works at the new rate)."""
    import torch

    x, clean, hz, injected = ref.science_case()
    D, T = x.shape
    spiky = x.copy()
    rng = np.random.default_rng(2)
    for d in range(D):
        spiky[d, rng.choice(T, 20, replace=False)] += 40.0
    flagged = make_tod({"signal": torch.as_tensor(spiky).to(DEV)}).flag_glitches(ctx=gpu_ctx)
    assert 0 < flagged.metadata["glitches"]["flagged_fraction"] < 0.02
    out = flagged.remove_lines(ctx=gpu_ctx)
    meta = out.metadata["lines"]
    assert torch.equal(out.flags, flagged.flags) and "glitches" in out.metadata
    assert meta["lines"][0].size == 2 and np.abs(meta["refined"] - hz).max() <= 1e-3 and meta["unfitted"] == 0
    floor = ref.noise_floor(2, meta["bounds"], T, 1.0, injected)
    keep = (out.flags == 0).cpu().numpy()
    resid = rms((out.data["signal"].cpu().numpy().astype(np.float64) - clean)[keep]) / injected
    print(f"behind flag_glitches: residual {resid / floor:.3f} x the floor on the unflagged samples")
    assert resid <= 1.5 * floor
    half = make_tod({"signal": torch.as_tensor(x.copy()).to(DEV)}).downsample(2, ctx=gpu_ctx)
    out = half.remove_lines(ctx=gpu_ctx)
    meta = out.metadata["lines"]
    assert meta["nperseg"] == 1024 and out.data["signal"].shape == (D, T // 2)
    found = meta["lines"][0]
    i = int(np.argmin(np.abs(found - ref.LINE_HZ[0])))  # the upper line sits in the decimator's transition band: it may be there or not
    assert abs(found[i] - ref.LINE_HZ[0]) < 50.0 / 1024 and np.abs(meta["refined"][:, i] - hz[:, 0]).max() <= 2e-3


def test_the_map_through_a_line(gpu_ctx):
    """A ProjectionMap source sampled on a constant-elevation scan, white noise, and a line of 2 sigma at 7.3137 Hz found
    by the finder with the sampled sky as the model.  The distance (rms over the hit pixels) of the BinMapper map from
    the map of the line-free TOD falls; by how much is asked of the host pipeline: the device-cleaned map is no further
    from the line-free one than twice the reference-cleaned map is."""
    import torch
    from test_gpu_downsample import _centre

    from maria_amd import lines
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.mappers import BinMapper
    from maria_amd.sim import TOD, Plan, Simulation, sky_transform_stack

    bands = [Band(center=93e9, width=27e9, shape="top_hat", name="f093"), Band(center=150e9, width=41e9, shape="top_hat", name="f150")]
    n, width = 128, 1.0  # degrees
    res = width / (n - 1)
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    data = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0
    data = (data - data.mean()).astype(np.float32)
    inst = Instrument(Detectors.hexagon(32, width / 2, bands, primary_size=30.0))
    site = Site(altitude=5000.0)
    plan = Plan.back_and_forth(start_time=1.7e9, duration=60.0, sample_rate=50.0, scan_center=(120.0, 55.0), throw=0.3, speed=0.5, accel=1.0)
    centre = _centre(plan.phi.astype(np.float32), plan.theta.astype(np.float32), sky_transform_stack(plan.time, site.latitude, site.longitude))
    sky = mmap.ProjectionMap(data, nu=150e9, width=width, center=np.degrees(centre), frame="ra/dec")
    (clean,) = Simulation(inst, plan, site, map=sky, noise=False).run()
    sky_field = torch.as_tensor(clean.data["map"]).to(DEV, torch.float32)
    D, T = sky_field.shape
    assert (D, T) == (64, 3000)
    sigma = 1e-3
    rng = np.random.default_rng(9)
    noise = torch.as_tensor((sigma * rng.standard_normal((D, T))).astype(np.float32)).to(DEV)
    fs = clean._sample_rate()
    lined = lines.inject_lines(noise, [7.3137], [2 * sigma], rng.uniform(-3, 3, (D, 1)), fs, ctx=gpu_ctx)
    meta = dict(clean.metadata)
    dirty = TOD({"map": sky_field, "noise": lined}, clean.dets, clean.coords, units="K_RJ", metadata=meta)
    cleaned = dirty.remove_lines(model=dirty.data["map"], into="noise", ctx=gpu_ctx)
    found = cleaned.metadata["lines"]["lines"]
    assert len(found) == 2 and all(v.size == 1 and abs(v[0] - 7.3137) < fs / 256 for v in found), found
    assert torch.equal(cleaned.data["map"], sky_field)
    signal = (sky_field + lined).cpu().numpy()
    y_ref, rec = ref.remove_lines(signal, lined.cpu().numpy(), fs, nperseg=256, groups=np.asarray(clean.dets.band_index), model=sky_field.cpu().numpy())
    assert all(v.size == 1 for v in rec["lines"])
    by_ref = TOD({"map": sky_field, "noise": torch.as_tensor(y_ref).to(DEV)}, clean.dets, clean.coords, units="K_RJ", metadata=meta)
    free = TOD({"map": sky_field, "noise": noise}, clean.dets, clean.coords, units="K_RJ", metadata=meta)
    maps = {}
    for name, tod in (("dirty", dirty), ("cleaned", cleaned), ("by_ref", by_ref), ("free", free)):
        mapper = BinMapper([tod], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="I",
                           nu=[b.center for b in bands], frame="ra/dec", units="K_RJ")
        maps[name] = np.asarray(mapper.run().data[0, :], np.float64)
    hit = ~np.isnan(maps["free"])
    assert hit.mean() > 0.05 and all(np.array_equal(np.isnan(m), ~hit) for m in maps.values())
    dist = {k: rms((maps[k] - maps["free"])[hit]) for k in ("dirty", "cleaned", "by_ref")}
    factor = dist["dirty"] / dist["by_ref"]
    print(f"map distance from the line-free map: with the line {dist['dirty']:.3e}, cleaned {dist['cleaned']:.3e}, cleaned by the reference "
          f"{dist['by_ref']:.3e} K_RJ: the reference gains a factor {factor:.2f}")
    assert factor > 2.0  # without this the test shows nothing
    assert dist["cleaned"] < dist["dirty"]
    assert dist["cleaned"] <= dist["dirty"] / (factor / 2.0)
