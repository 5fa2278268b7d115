"""mrx_tod_segment_project, maria_amd.subscans.freeze / project / Projector and MaximumLikelihoodMapper(subscan_filter=...)
on the device.

The entry is pinned to the bit by the two entries it fuses: its coefficients are the ordered product A r of
tests/subscan_project_ref.py with r from mrx_tod_segment_normal, and its output is mrx_tod_segment_apply of those
coefficients.  Against the dense float64 F it is held to the two float32 roundings of its last step
(tests/test_host_subscan_project.py: dense_case).  The mapper is compared with dense float64 solves and with the plain map
on a blob under polynomial drifts."""

import numpy as np
import pytest
import subscan_project_ref as pref
import subscans_ref as ref
from test_gpu_flagging import device_rows, untouched_outside
from test_gpu_subscans import LENGTHS, ROWS, bits, make_bounds

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T_ALL = sum(LENGTHS) + 11  # every length fits between the samples in no segment at both ends


def case(D, K, flagged, seed):
    """(x, flags, bounds): Gaussian rows over every length of LENGTHS in a random order; ``flagged`` of the samples flagged
    (values 1 and 2) and, in the last row, the first segment of 255 or more samples wholly."""
    rng = np.random.default_rng(seed)
    bounds = make_bounds(T_ALL, seed)
    assert sorted(np.diff(bounds).tolist()) == sorted(LENGTHS) and bounds[0] > 0 and bounds[-1] < T_ALL
    x = (rng.standard_normal((D, T_ALL)) * 3 + 5).astype(np.float32)
    flags = ((rng.random((D, T_ALL)) < flagged) * rng.integers(1, 3, (D, T_ALL))).astype(np.uint8)
    if flagged:
        s = int(np.flatnonzero(np.diff(bounds) >= 255)[0])
        flags[D - 1, bounds[s]:bounds[s + 1]] = 2
    return x, flags, bounds


def frozen(gpu_ctx, xv, bounds, K, fv, min_hits=8):
    from maria_amd import subscans

    N, _, hits = subscans.normal_equations(xv, bounds, K, flags=fv, ctx=gpu_ctx)
    return subscans.freeze(N, hits, min_hits=min_hits)


def expected(gpu_ctx, x, bounds, K, flags, A, ok, transpose):
    """(a, y) the entry must give, from the two entries it fuses: r of mrx_tod_segment_normal (with the flags forward,
    without them transposed), the ordered A r on the host, mrx_tod_segment_apply of it (kept where flagged, transposed)."""
    import torch

    from maria_amd import subscans

    dx = torch.as_tensor(x).to(DEV)
    df = None if flags is None else torch.as_tensor(flags).to(DEV)
    _, r, _ = subscans.normal_equations(dx, bounds, K, flags=None if transpose else df, ctx=gpu_ctx)
    okh = ok.cpu().numpy() != 0
    a = pref.ordered_product(A.cpu().numpy(), np.where(okh[:, :, None], r.cpu().numpy(), 0.0))
    y = subscans.apply(dx, bounds, torch.as_tensor(a).to(DEV), -1, ctx=gpu_ctx).cpu().numpy()
    if transpose and flags is not None:
        y = np.where(flags == 0, y, x)
    covered = np.zeros((x.shape[0], x.shape[1]), bool)
    for s, (lo, hi) in enumerate(ref.segments(bounds, x.shape[1])):
        covered[:, lo:hi] = okh[:, s, None]
    return a, np.where(covered, y, x)  # a pair that is not ok keeps its bits (x - 0.0f would too, but for a NaN's payload)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("K", range(1, 9))
def test_the_entry_is_the_two_it_fuses_bit_for_bit(gpu_ctx, K, transpose):
    """Rows 1, 3 and 33, every length 0 .. 2049 in a random order with samples in no segment, flags at 0 % and 30 % with a
    wholly flagged segment, plain and padded odd pitches, min_hits 8 and 0 (the short segments fitted too): d_a and x bit
    for bit, the inputs unchanged, nothing written outside the rows."""
    import torch

    from maria_amd import subscans

    for i, D in enumerate(ROWS):
        for flagged in (0.0, 0.3):
            padded = (i + K + (flagged > 0)) % 2 == 0
            x, flags, bounds = case(D, K, flagged, 100 * K + 10 * D + (flagged > 0))
            T = x.shape[1]
            xbuf, xv = device_rows(x, T + 3, 1, -3.0) if padded else device_rows(x, T, 0, -3.0)
            fbuf, fv = device_rows(flags, T + 1, 1, 9) if padded else device_rows(flags, T, 0, 9)
            if not flagged and i % 2 == 0:
                fv = None  # d_flags NULL: nothing is flagged
            A, ok = frozen(gpu_ctx, xv, bounds, K, fv, min_hits=8 if (i + K) % 2 else 0)
            okh = ok.cpu().numpy() != 0
            lengths = np.diff(bounds)
            assert okh[:, lengths >= 63].sum() >= D * 8 - 1 and not okh[:, lengths == 0].any() and (not flagged or not okh.all())
            want_a, want_y = expected(gpu_ctx, x, bounds, K, flags if fv is not None else None, A, ok, transpose)
            fbefore = fbuf.clone()
            out, a = subscans.project(xv, bounds, A, ok, flags=fv, transpose=transpose, coefficients=True, ctx=gpu_ctx)
            torch.cuda.synchronize()
            where = (K, transpose, D, flagged, padded)
            assert out is xv and torch.equal(fbuf, fbefore), where
            assert np.array_equal(bits(a.cpu().numpy()), bits(want_a)), where
            assert not a.cpu().numpy()[~okh].any() and np.abs(want_a[okh]).min() > 0
            assert np.array_equal(bits(xv.cpu().numpy()), bits(want_y)), where
            assert not np.array_equal(want_y, x)
            assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"


@pytest.mark.parametrize("K", range(1, 9))
def test_against_the_dense_float64_operator(gpu_ctx, K):
    """Rows of 3 x 257 samples, 30 % flagged, F and F^t: every sample within 2^-24 (|p64| + |y64|) plus the reference's
    own float64 error (x 4) of the dense float64 operator (tests/test_host_subscan_project.py: dense_case, where the
    reference through the same two roundings is shown to stay inside this bound)."""
    import torch
    from test_host_subscan_project import dense_case

    from maria_amd import subscans

    for transpose in (0, 1):
        x, flags, bounds, y64, bound, _ = dense_case(K, transpose)
        xv, fv = torch.as_tensor(x).to(DEV), torch.as_tensor(flags).to(DEV)
        A, ok = frozen(gpu_ctx, xv, bounds, K, fv)
        assert bool(ok.all())
        subscans.project(xv, bounds, A, ok, flags=fv, transpose=bool(transpose), ctx=gpu_ctx)
        ratio = float((np.abs(xv.cpu().numpy().astype(np.float64) - y64) / bound).max())
        print(f"K {K} transpose {transpose}: max |y - dense| / bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("K", [1, 4, 8])
def test_the_two_calls_are_adjoint(gpu_ctx, K):
    """<F x, y> against <x, F^t y> between the two device calls, in test_gpu_filter_aware's form: the gap is at most
    STEP_TOL (one float32-rounded step) times sum over rows of max|F x| |y|_1 + max|F^t y| |x|_1."""
    import torch
    from test_gpu_filter_aware import STEP_TOL

    from maria_amd import subscans

    x, flags, bounds = case(33, K, 0.3, 7 + K)
    y = np.random.default_rng(K).standard_normal(x.shape).astype(np.float32)
    fv = torch.as_tensor(flags).to(DEV)
    A, ok = frozen(gpu_ctx, torch.as_tensor(x).to(DEV), bounds, K, fv)
    Fx = subscans.project(torch.as_tensor(x).to(DEV), bounds, A, ok, flags=fv, ctx=gpu_ctx).cpu().numpy().astype(np.float64)
    Fty = subscans.project(torch.as_tensor(y).to(DEV), bounds, A, ok, flags=fv, transpose=True, ctx=gpu_ctx).cpu().numpy().astype(np.float64)
    gap = abs(np.sum(Fx * y) - np.sum(x * Fty))
    bound = STEP_TOL * np.sum(np.abs(Fx).max(axis=1) * np.abs(y).sum(axis=1) + np.abs(Fty).max(axis=1) * np.abs(x).sum(axis=1))
    print(f"K {K}: adjoint gap {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound


def test_what_is_not_fitted_keeps_every_bit(gpu_ctx):
    """NaN and -0.0 in the pairs that are not ok and in the samples in no segment: every bit kept, in both modes; the pairs'
    d_a zero; the padding of a padded row keeps its sentinel."""
    import torch

    from maria_amd import subscans

    K = 3
    x, flags, bounds = case(3, K, 0.3, 5)
    T = x.shape[1]
    fv = torch.as_tensor(flags).to(DEV)
    A, ok = frozen(gpu_ctx, torch.as_tensor(x).to(DEV), bounds, K, fv)
    okh = ok.cpu().numpy() != 0
    quiet = np.ones((3, T), bool)  # the samples of no fitted pair
    for s, (lo, hi) in enumerate(ref.segments(bounds, T)):
        quiet[:, lo:hi] = ~okh[:, s, None]
    assert quiet[:, :2].all() and quiet[:, -3:].all() and quiet[2].sum() > 255 + 11
    x[quiet] = np.where(np.arange(quiet.sum()) % 2 == 0, np.float32("nan"), np.float32(-0.0))
    for transpose in (False, True):
        xbuf, xv = device_rows(x, T + 5, 3, -3.0)
        _, a = subscans.project(xv, bounds, A, ok, flags=fv, transpose=transpose, coefficients=True, ctx=gpu_ctx)
        got = xv.cpu().numpy()
        assert np.array_equal(bits(got[quiet]), bits(x[quiet])) and not np.array_equal(bits(got[~quiet]), bits(x[~quiet]))
        assert np.isfinite(got[~quiet]).all() and not a.cpu().numpy()[~okh].any()
        assert untouched_outside(xbuf, xv, -3.0)


def test_junk_under_the_flags_and_an_unflagged_nan(gpu_ctx):
    """Forward: 1e30 or NaN under the flags changes no bit of d_a and no bit of any unflagged output.  An unflagged NaN
    stays inside its own (row, segment), in both modes."""
    import torch

    from maria_amd import subscans

    K = 6
    x, flags, bounds = case(33, K, 0.3, 31)
    fv = torch.as_tensor(flags).to(DEV)
    A, ok = frozen(gpu_ctx, torch.as_tensor(x).to(DEV), bounds, K, fv)
    results = []
    for fill in (None, 1e30, float("nan")):
        xx = x.copy()
        if fill is not None:
            xx[flags != 0] = fill
        y, a = subscans.project(torch.as_tensor(xx).to(DEV), bounds, A, ok, flags=fv, coefficients=True, ctx=gpu_ctx)
        results.append((a.cpu().numpy(), y.cpu().numpy()[flags == 0]))
    assert np.isfinite(results[0][0]).all()
    for other in results[1:]:
        assert np.array_equal(bits(results[0][0]), bits(other[0])) and np.array_equal(bits(results[0][1]), bits(other[1]))
    s = int(np.flatnonzero(np.diff(bounds) == 1025)[0])
    t = int(bounds[s]) + int(np.flatnonzero(flags[4, bounds[s]:bounds[s + 1]] == 0)[7])
    for transpose in (False, True):
        clean = subscans.project(torch.as_tensor(x).to(DEV), bounds, A, ok, flags=fv, transpose=transpose, ctx=gpu_ctx).cpu().numpy()
        xx = x.copy()
        xx[4, t] = np.nan
        y, a = subscans.project(torch.as_tensor(xx).to(DEV), bounds, A, ok, flags=fv, transpose=transpose, coefficients=True, ctx=gpu_ctx)
        y, a = y.cpu().numpy(), a.cpu().numpy()
        own = np.zeros(x.shape, bool)
        own[4, bounds[s]:bounds[s + 1]] = True
        assert np.array_equal(bits(y[~own]), bits(clean[~own])) and np.isnan(y[4, t]) and np.isnan(a[4, s]).all()
        assert np.isfinite(np.delete(a.reshape(-1, K), 4 * (len(bounds) - 1) + s, axis=0)).all()


def test_the_same_bits_alone_and_at_either_alignment(gpu_ctx):
    """The same bits on a second call, for a row alone, for a segment alone (its own two bounds, its own A and ok), at
    either alignment, and with other rows added, in both modes."""
    import torch

    from maria_amd import subscans

    for K, transpose in ((1, False), (4, True), (5, False), (8, True)):
        x, flags, bounds = case(33, K, 0.3, 8 + K)
        T = x.shape[1]
        S = len(bounds) - 1
        fv = torch.as_tensor(flags).to(DEV)
        A, ok = frozen(gpu_ctx, torch.as_tensor(x).to(DEV), bounds, K, fv)

        def run(xs, fs, bs, As, oks):
            y, a = subscans.project(xs, bs, As, oks, flags=fs, transpose=transpose, coefficients=True, ctx=gpu_ctx)  # noqa: B023
            return y.cpu().numpy(), a.cpu().numpy()

        first = run(torch.as_tensor(x).to(DEV), fv, bounds, A, ok)
        again = run(torch.as_tensor(x).to(DEV), fv, bounds, A, ok)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again))
        for row in (0, 16, 32):
            y, a = run(torch.as_tensor(x[row:row + 1]).to(DEV), fv[row:row + 1], bounds, A[row:row + 1], ok[row:row + 1])
            assert np.array_equal(bits(y), bits(first[0][row:row + 1])) and np.array_equal(bits(a), bits(first[1][row:row + 1])), (K, row)
        for s in range(S):
            y, a = run(torch.as_tensor(x).to(DEV), fv, bounds[s:s + 2], A[:, s:s + 1], ok[:, s:s + 1])
            lo, hi = bounds[s], bounds[s + 1]
            assert np.array_equal(bits(y[:, lo:hi]), bits(first[0][:, lo:hi])) and np.array_equal(bits(a), bits(first[1][:, s:s + 1])), (K, s)
            assert np.array_equal(bits(y[:, :lo]), bits(x[:, :lo])) and np.array_equal(bits(y[:, hi:]), bits(x[:, hi:]))
        for pitch, offset in ((T + (-T) % 4, 0), (T + 1 + (-(T + 1)) % 2, 1)):
            got = run(device_rows(x, pitch, offset, 0)[1], device_rows(flags, pitch + 2, offset, 0)[1], bounds, A, ok)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, got)), (K, pitch)
        more = np.concatenate([x[20:], x])  # the rows behind 13 others
        y, a = run(torch.as_tensor(more).to(DEV), torch.cat([fv[20:], fv]), bounds, torch.cat([A[20:], A]), torch.cat([ok[20:], ok]))
        assert np.array_equal(bits(y[13:]), bits(first[0])) and np.array_equal(bits(a[13:]), bits(first[1]))


def test_hostile_bounds_are_clamped(gpu_ctx):
    """The C entry with bounds below 0, above T and reversed, sentinel rows around the buffer: clamped, a reversed pair
    empty, nothing out of range.  (Segments that overlap are the caller's business: the pairs of this call are kept apart
    by d_ok.)  Through the Python side, whose bounds ascend: clamped at both ends and the entry's usual bits."""
    import torch

    from maria_amd import subscans
    from maria_amd._lib import ptr

    D, T, K = 3, 300, 4
    rng = np.random.default_rng(21)
    x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
    flags = (rng.random((D, T)) < 0.1).astype(np.uint8)
    flags[:, :8] = 0  # [0, 5) keeps its five samples
    raw = np.array([-2**31, -7, 5, 3, 3, 140, 120, T + 9, 2**31 - 1], np.int32)  # [0, 0) [0, 5) [5, 3) [3, 3) [3, 140) [140, 120) [120, 300) [300, 300)
    S = len(raw) - 1
    assert [hi - lo for lo, hi in ref.segments(raw, T)] == [0, 5, -2, 0, 137, -20, 180, 0]
    d_raw = torch.as_tensor(raw).to(DEV)
    xbuf, xv = device_rows(x, T + 3, T + 3 + 1, -3.0)  # a sentinel row in front, the buffer's spare words behind
    fbuf, fv = device_rows(flags, T + 1, 1, 9)
    for live in ([4], [1, 6], []):  # [3, 140) alone; [0, 5) and [120, 300), which do not meet; none
        N = torch.empty((D, S, K, K), dtype=torch.float64, device=DEV)
        r = torch.empty((D, S, K), dtype=torch.float64, device=DEV)
        hits = torch.empty((D, S), dtype=torch.int32, device=DEV)
        xv.copy_(torch.as_tensor(x))
        gpu_ctx.call("mrx_tod_segment_normal", ptr(xv), T + 3, None, 0, ptr(fv), T + 1, D, T, ptr(d_raw), S, K, ptr(N), ptr(r), ptr(hits))
        A, ok = subscans.freeze(N, hits.to(torch.int64), min_hits=4)
        keep = torch.zeros((D, S), dtype=torch.uint8, device=DEV)
        keep[:, live] = 1
        ok = ok & keep
        assert ok.cpu().numpy()[:, live].all()
        a = torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV)
        gpu_ctx.call("mrx_tod_segment_project", ptr(xv), T + 3, ptr(fv), T + 1, D, T, ptr(d_raw), S, K, ptr(A), ptr(ok), 0, ptr(a))
        torch.cuda.synchronize()
        want = x.copy()
        for s in live:
            lo, hi = ref.segments(raw, T)[s]
            pair = np.array([lo, hi], np.int32)
            a_s = pref.ordered_product(A[:, s].cpu().numpy(), r[:, s].cpu().numpy())
            assert np.array_equal(bits(a[:, s].cpu().numpy()), bits(a_s))
            want[:, lo:hi] = ref.apply(x, pair, a_s[:, None, :])[:, lo:hi]
        got = xv.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)) and (not live or not np.array_equal(got, x))
        dead = [s for s in range(S) if s not in live]
        assert not a.cpu().numpy()[:, dead].any()
        assert untouched_outside(xbuf, xv, -3.0) and bool((fv.cpu() == torch.as_tensor(flags)).all())
    asc = np.array([-7, 5, 5, 140, T + 9], np.int32)
    xbuf, xv = device_rows(x, T + 3, T + 3 + 1, -3.0)
    A, ok = frozen(gpu_ctx, xv, asc, K, fv, min_hits=4)
    assert ok.cpu().numpy().tolist() == [[1, 0, 1, 1]] * D
    want_a, want_y = expected(gpu_ctx, x, asc, K, flags, A, ok, False)
    _, a = subscans.project(xv, asc, A, ok, flags=fv, coefficients=True, ctx=gpu_ctx)
    assert np.array_equal(bits(a.cpu().numpy()), bits(want_a)) and np.array_equal(bits(xv.cpu().numpy()), bits(want_y))
    assert untouched_outside(xbuf, xv, -3.0)


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves x and d_a untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T, S, K = 4, 3000, 3, 3
    x = torch.ones((D, T + 4), dtype=torch.float32, device=DEV)
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    bound = torch.as_tensor(np.array([0, 1000, 1000, T], np.int32)).to(DEV)
    A = torch.zeros((D, S, K, K), dtype=torch.float64, device=DEV)
    A[:, :, 0, 0] = 1.0 / 1000.0
    ok = torch.ones((D, S), dtype=torch.uint8, device=DEV)
    a = torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    good = (ptr(x), T + 4, ptr(flags), T, D, T, ptr(bound), S, K, ptr(A), ptr(ok), 0, ptr(a))

    def put(*pairs):
        args = list(good)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    bad = {"null x": put((0, None)), "null bound": put((6, None)), "null A": put((9, None)), "null ok": put((10, None)), "D 0": put((4, 0)),
           "T 0": put((5, 0)), "S 0": put((7, 0)), "S -1": put((7, -1)), "K 0": put((8, 0)), "K 9": put((8, 9)), "transpose 2": put((11, 2)),
           "transpose -1": put((11, -1)), "ld_x < T": put((1, T - 1)), "ld_f < T": put((3, T - 1))}
    for name, args in bad.items():
        assert lib.mrx_tod_segment_project(hd, *args) == -1, name
        assert b"mrx_tod_segment_project" in lib.mrx_last_error(hd), name
    torch.cuda.synchronize()
    assert bool((x == 1.0).all()) and bool((a == 7.0).all())
    # a pitch of flags that are not given is not looked at; d_a may be null
    assert lib.mrx_tod_segment_project(hd, *put((2, None), (3, 0), (12, None))) == 0
    torch.cuda.synchronize()
    # A = e_0 e_0^t / 1000 on ones: r_0 = 1000 (2000), a = (1, 0, 0) ((2, 0, 0)): 1 - 1 and 1 - 2; the second segment is empty
    assert bool((x[:, :1000] == 0.0).all()) and bool((x[:, 1000:T] == -1.0).all()) and bool((x[:, T:] == 1.0).all()) and bool((a == 7.0).all())
    assert lib.mrx_tod_segment_project(hd, *put((11, 1))) == 0
    torch.cuda.synchronize()
    assert not bool(a[:, 1].any()) and bool((a[:, 0] != 7.0).all())


@pytest.mark.parametrize("transpose", [0, 1])
def test_past_the_first_trip_of_the_resident_grid(gpu_ctx, transpose):
    """D S / 4 >= 2 R + R / 2 + 1 workgroups, R = 8 n_cu (tests/test_gpu_resident_trips.py: wave_shape, asserted there):
    the whole output, padding included, equals the same call on blocks of rows small enough for one trip, bit for bit."""
    import torch
    from test_gpu_resident_trips import WAVES, on_device, place, resident, wave_shape

    from maria_amd import subscans
    from maria_amd._lib import ptr

    n_cu, R, D, S, T, bounds, n_groups = wave_shape(gpu_ctx)
    assert n_groups >= resident(gpu_ctx)[2]
    K = 3
    rng = np.random.default_rng(D + transpose)
    x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
    flags = (rng.random((D, T)) < 0.1).astype(np.uint8)
    fbuf, fv, ld_f = place(flags, "odd", 9)
    d_bound = on_device(bounds)
    N, _, hits = subscans.normal_equations(on_device(x), bounds, K, flags=fv, ctx=gpu_ctx)
    A, ok = subscans.freeze(N, hits, min_hits=4)
    assert 0.5 < float(ok.float().mean()) < 1.0
    outs = []
    for step in (D, D, max(1, WAVES * n_cu // S)):
        xbuf, xv, ld_x = place(x, "odd", -3.0)
        a = torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV)
        for lo in range(0, D, step):
            hi = min(D, lo + step)
            gpu_ctx.call("mrx_tod_segment_project", ptr(xv[lo:hi]), ld_x, ptr(fv[lo:hi]), ld_f, hi - lo, T, ptr(d_bound), S, K, ptr(A[lo:hi]),
                         ptr(ok[lo:hi]), transpose, ptr(a[lo:hi]))
        torch.cuda.synchronize()
        outs.append((xbuf, a))
    for other in outs[1:]:
        assert torch.equal(outs[0][0], other[0]) and torch.equal(outs[0][1], other[1])
    assert not torch.equal(outs[0][0][1:1 + T], torch.as_tensor(x[0]).to(DEV))


# ---- the mapper ---------------------------------------------------------------------------------

BOUNDS = np.arange(0, 6001, 300).astype(np.int32)


def _flags(D, T, seed, fraction=0.1):
    return (np.random.default_rng(seed).random((D, T)) < fraction).astype(np.uint8)


def dense_system(gpu_ctx, modes):
    """(mapper, map, A, b, shape): test_gpu_filter_aware.test_map_matches_a_dense_solve's set-up with subscan_filter = order 3
    in segments of 300 samples and 10 % of the samples flagged, alone or in front of MODES_CONFIG, and the float64 dense
    system of it: F = F_pre F' from the references and the mapper's reported products, W the mapper's 1 / var weights
    times (flags == 0)."""
    import filter_aware_ref as fa
    import torch
    from test_gpu_filter_aware import MODES_CONFIG, _copy, _pointing_matrix, _signal_for
    from test_gpu_noise_filter import _tods

    from maria_amd import subscans
    from maria_amd import tod_processing as tp
    from maria_amd.mappers import MaximumLikelihoodMapper
    from maria_amd.tod import field_sum

    tod, az, el = _tods()
    D, T = tod.dets.n, tod.coords.t.size
    config = _copy(MODES_CONFIG) if modes else {}
    kw = dict(center=(az, el), width=16 * 0.05, height=12 * 0.05, resolution=0.05, stokes="IQU", frame="az/el", tol=1e-8, max_iter=400)
    probe = MaximumLikelihoodMapper([tod], **kw)
    shape = (3, 1, probe.n_eta, probe.n_xi)
    assert shape[2:] == (12, 16)
    P = _pointing_matrix(probe, tod, shape)
    tod.data = {"map": _signal_for(P, shape, D, T, seed=9)}
    tod.flags = _flags(D, T, 4)
    spec = {"order": 3, "bounds": BOUNDS}
    mapper = MaximumLikelihoodMapper([tod], tod_preprocessing=_copy(config), filter_aware=True, subscan_filter=spec, **kw)
    m = mapper.run().data
    assert mapper.products["converged"] and mapper.products["filter_aware"] is True
    (pre,) = mapper.products["preprocessing"]
    assert pre["steps"] == ["filter_subscans"] + (["filter", "remove_modes"] if modes else [])
    sub = pre["subscans"]
    assert sub["order"] == 3 and sub["bounds"].tolist() == BOUNDS.tolist() and sub["unfitted"].shape == (0, 2)
    frozen_ref = pref.Frozen(D, T, BOUNDS, 4, tod.flags, unfitted=sub["unfitted"])
    steps = fa.build(_copy(config), tod.coords.t, modes=(pre["modes"], pre["row_norms"])) if modes else []
    F = lambda v: fa.apply(steps, frozen_ref.apply(v)) if steps else frozen_ref.apply(v)  # noqa: E731
    # the mapper's weight: 1 / var of every row after F' and the recorded steps (the same calls, the same bits)
    rows = field_sum(tod.data.values(), torch.device(DEV))
    d_flags = torch.as_tensor(tod.flags).to(DEV)
    subscans.Projector(rows, BOUNDS, 4, flags=d_flags, ctx=gpu_ctx).apply(rows)
    rows = tp.process_tod(tod._derived(data={"total": rows}), config=_copy(config), ctx=gpu_ctx, device=DEV).data["total"]
    w = ((1.0 / rows.double().var(dim=1)).cpu().numpy()[:, None] * (tod.flags == 0)).ravel()
    n = P.shape[1]
    FP = np.empty((D * T, n))
    Pc = P.tocsc()
    for j in range(n):
        FP[:, j] = F(Pc[:, j].toarray().reshape(D, T)).ravel()
    Fd = F(tod.data["map"].astype(np.float64)).ravel()
    WFP = FP * w[:, None]
    return mapper, m, FP.T @ WFP, WFP.T @ Fd, shape


@pytest.mark.parametrize("modes", [False, True])
def test_map_matches_a_dense_solve(gpu_ctx, modes):
    """The map equals the float64 dense solve of (P^T F^T W F P) m = P^T F^T W F d (``dense_system``) within
    test_gpu_filter_aware.test_map_matches_a_dense_solve's 1e-6, each plane up to its hits-weighted mean as there.

    The precondition, a condition number <= 1e8 on the solved pixels, is asserted on the complement of the three plane
    constants.  Those are an exact null space for every order: a constant I, Q or U map is a constant in every detector row
    (every sample of this set-up falls on the map), a multiple of P_0, and F' T = 0.  Measured: |A c| <= 1.2e-16 of the
    largest eigenvalue for the three constants c, the three lowest eigenvalues 4e-14 .. 1e-12 with eigenvectors constant
    in each plane to 1e-15, and on the complement a condition number of 6.2e3 alone and 1.0e4 in front of MODES_CONFIG.
    The comparison never saw those three directions (the hits-weighted means); the dense solve is made on the
    complement, where it is well posed."""
    mapper, m, A, b, shape = dense_system(gpu_ctx, modes)
    n = int(np.prod(shape))
    solved = np.isfinite(m).ravel()
    assert solved.sum() >= 0.8 * n, solved.sum() / n
    As, bs = A[np.ix_(solved, solved)], b[solved]
    plane = np.repeat(np.arange(shape[0]), n // shape[0])[solved]
    C = np.stack([(plane == s) / np.sqrt((plane == s).sum()) for s in range(shape[0])], axis=1)
    top = float(np.linalg.eigvalsh(As)[-1])
    null = float(np.abs(As @ C).max() / top)
    Q = np.linalg.qr(np.concatenate([C, np.random.default_rng(0).normal(size=(As.shape[0], As.shape[0] - shape[0]))], axis=1))[0][:, shape[0]:]
    assert np.abs(Q.T @ C).max() <= 1e-12
    Aq = Q.T @ As @ Q
    eig = np.linalg.eigvalsh(Aq)
    cond = float(eig[-1] / eig[0])
    print(f"[subscan filter] modes {modes}: |A c| / |A| = {null:.2e} for the plane constants; condition number on their complement {cond:.3e}")
    assert null <= 1e-12 and eig[0] > 0 and cond <= 1e8
    dense = np.full(n, np.nan)
    dense[solved] = Q @ np.linalg.solve(Aq, Q.T @ bs)
    dense, got = dense.reshape(shape), m.astype(np.float64)
    w = mapper.products["weight"][0, 0]
    err, scale = 0.0, 0.0
    for s in range(shape[0]):  # test_gpu_filter_aware._compare_with_dense's comparison
        ok = np.isfinite(got[s, 0])
        r = got[s, 0][ok] - dense[s, 0][ok]
        r -= np.sum(w[ok] * r) / np.sum(w[ok])
        d0 = dense[s, 0][ok] - np.sum(w[ok] * dense[s, 0][ok]) / np.sum(w[ok])
        err = max(err, np.abs(r).max())
        scale = max(scale, np.abs(d0).max())
    err /= scale
    print(f"[subscan filter] dense solve (modes {modes}): max |map - dense| / max |dense| = {err:.2e}, {mapper.products['n_iter']} iterations, "
          f"|r|/|b| {mapper.products['residuals'][-1]:.1e}")
    assert err <= 1e-6, err


def _blob_tod(order, flagged, seed):
    """test_extended_emission_survives_the_filter's fixture (24 x 6000 at 50 Hz, a 16 x 16 nearest I map, a unit blob of
    sigma 0.45, white noise of 0.01) under Legendre drifts of unit-rms coefficients per (detector, segment of 300): (tod,
    truth, mapper keywords)."""
    from test_gpu_noise_filter import _project, _tods

    from maria_amd.mappers import MaximumLikelihoodMapper

    D, T = 24, 6000
    tod, az, el = _tods(D=D, T=T, angles=(0.0,))
    kw = dict(center=(az, el), width=16 * 0.05, resolution=0.05, stokes="I", frame="az/el", max_iter=100)
    probe = MaximumLikelihoodMapper([tod], **kw)
    assert (probe.n_eta, probe.n_xi) == (16, 16)
    E, X = np.meshgrid(np.linspace(-1, 1, 16), np.linspace(-1, 1, 16), indexing="ij")
    truth = np.exp(-0.5 * (E**2 + X**2) / 0.45**2)
    rng = np.random.default_rng(seed)
    drift = ref.fit_values(BOUNDS, rng.standard_normal((D, len(BOUNDS) - 1, order + 1)), T)
    d = _project(probe, tod, truth.reshape(1, 1, 16, 16)).cpu().numpy().astype(np.float64) + drift + 0.01 * rng.normal(size=(D, T))
    tod.data = {"map": d.astype(np.float32)}
    if flagged:
        tod.flags = _flags(D, T, seed + 1, flagged)
    return tod, truth, kw


def _rms_error(mapper, truth):
    m = mapper.run().data[0, 0].astype(np.float64)
    hits = mapper.products["weight"][0, 0]
    ok = np.isfinite(m)
    r = m[ok] - truth[ok]
    r -= np.sum(hits[ok] * r) / np.sum(hits[ok])
    return float(np.sqrt(np.mean(r**2))), int(ok.sum())


@pytest.mark.parametrize("flagged", [0.0, 0.1])
@pytest.mark.parametrize("order", [1, 3])
def test_extended_emission_survives_the_subscan_filter(gpu_ctx, order, flagged):
    """The blob under polynomial drifts, through TOD.filter_subscans(bounds=...) (the turnarounds of the daisy scan not
    flagged: 0 % or 10 % of the samples are): the rms error of the map of filter_aware=True, subscan_filter="recorded",
    hits-weighted mean removed, is at most a tenth of the plain MaximumLikelihoodMapper map's of the same TOD, converged
    within 100 iterations.  (A float64 restatement with tangent-plane pointing: 1/130 .. 1/280 in 10 .. 23 iterations.)"""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, truth, kw = _blob_tod(order, flagged, 10 * order + int(10 * flagged))
    filtered = tod.filter_subscans(order=order, bounds=BOUNDS, flag_turnarounds=False, ctx=gpu_ctx)
    assert filtered.metadata["subscans"]["failed_segments"].shape == (0, 2)
    e_plain, n_plain = _rms_error(MaximumLikelihoodMapper([filtered], **kw), truth)
    aware = MaximumLikelihoodMapper([filtered], filter_aware=True, subscan_filter="recorded", **kw)
    e_aware, n_aware = _rms_error(aware, truth)
    print(f"[subscan filter] order {order}, {flagged:.0%} flagged: rms error plain {e_plain:.4f}, filter-aware {e_aware:.5f} "
          f"(ratio 1/{e_plain / e_aware:.1f}) over {n_aware} pixels, {aware.products['n_iter']} iterations")
    assert n_aware == n_plain and n_aware > 0
    assert aware.products["converged"] and aware.products["n_iter"] <= 100
    assert aware.products["preprocessing"][0]["subscans"]["order"] == order
    assert e_aware <= 0.1 * e_plain, (e_aware, e_plain)


def test_the_second_projection_changes_nothing(gpu_ctx):
    """F' F = F' on the device: the same map, to the solve's tolerance (tol 1e-8; 1e-6 of the map's maximum, the bound of
    test_gpu_filter_aware.test_no_preprocessing_is_the_plain_map), whether the TOD went through filter_subscans first (with
    fewer flags than it has now) or is handed over unfiltered with the dict form.  Uniform weights: 1 / var of rows
    that differ by float32 roundings would differ too."""
    import torch

    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, truth, kw = _blob_tod(3, 0.05, 77)
    kw = dict(kw, tol=1e-8, noise_weights="uniform")
    filtered = tod.filter_subscans(order=3, bounds=BOUNDS, flag_turnarounds=False, ctx=gpu_ctx)
    later = torch.as_tensor(filtered.flags).cpu().numpy() | _flags(24, 6000, 78, 0.05)  # more was flagged after the filter
    filtered.flags = later
    tod.flags = later
    first = MaximumLikelihoodMapper([filtered], filter_aware=True, subscan_filter="recorded", **kw)
    second = MaximumLikelihoodMapper([tod], filter_aware=True, subscan_filter={"order": 3, "bounds": BOUNDS}, **kw)
    a, b = first.run().data, second.run().data
    assert first.products["converged"] and second.products["converged"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = np.isfinite(a)
    err = float(np.abs(a[ok] - b[ok]).max() / np.abs(a[ok]).max())
    print(f"[subscan filter] filtered first or not: max |difference| / max |map| = {err:.2e}")
    assert err <= 1e-6


def test_the_map_does_not_see_what_is_under_the_flags(gpu_ctx):
    """1e30 under the flags changes no bit of the map (uniform weights: 1 / var of a row looks at every sample)."""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, truth, kw = _blob_tod(2, 0.1, 55)
    kw = dict(kw, noise_weights="uniform", filter_aware=True, subscan_filter={"order": 2, "bounds": BOUNDS})
    clean = MaximumLikelihoodMapper([tod], **kw).run().data
    junk = tod.data["map"].copy()
    junk[tod.flags != 0] = 1e30
    tod.data = {"map": junk}
    dirty = MaximumLikelihoodMapper([tod], **kw).run().data
    assert np.isfinite(clean).sum() > 100 and np.array_equal(bits(clean), bits(dirty))


@pytest.mark.parametrize("filter_aware", [False, True])
def test_the_default_is_the_path_it_was(gpu_ctx, filter_aware):
    """subscan_filter=None spelled out or left out, with a pre-processing configured, filter-aware or not: the same
    products, no new key, and bit for bit everything that repeats bit for bit at all: what the mapper makes of the TOD (the
    signal it bins, the weight, the operator's steps, modes and row norms).

    The maps of two runs of ONE configuration are not the same bits on this code, with or without this keyword: the map
    sums are float64 atomics.  Measured between runs of the configuration with the keyword left out:
    rhs, blocks and weight differ by up to 1.1e-15 of their maximum, the plain map by 1.5e-15, the filter-aware map by up
    to 9.1e-9 and its residuals by 3.4e-9 (conjugate gradients carry the difference along).  So the float64 sums are held
    to 1e-12 of their maximum (a thousand times the measured order effect, a millionth of what a changed float32 signal
    would do), the plain map to the same bits in float32 (as test_gpu_filter_aware does) and the filter-aware map to the
    solve's tolerance, 1e-6 of its maximum."""
    import torch
    from test_gpu_filter_aware import MODES_CONFIG, _copy, _noisy_tod

    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, kw = _noisy_tod()
    kw = dict(kw, tod_preprocessing=_copy(MODES_CONFIG), filter_aware=filter_aware)
    left_out = MaximumLikelihoodMapper([tod], **kw)
    spelled = MaximumLikelihoodMapper([tod], subscan_filter=None, **kw)
    assert left_out.subscan_filter is None and spelled.subscan_filter is None
    made = [mp._tod_inputs(tod, gpu_ctx, unit_i_response=True, with_operator=filter_aware) for mp in (left_out, spelled)]
    if filter_aware:
        (ia, oa), (ib, ob) = made
        pa, pb = oa.product(), ob.product()
        assert pa["steps"] == pb["steps"] == ["filter", "remove_modes"] and "subscans" not in pb
        assert np.array_equal(bits(pa["modes"]), bits(pb["modes"])) and np.array_equal(bits(pa["row_norms"]), bits(pb["row_norms"]))
    else:
        ia, ib = made
    assert torch.equal(ia.signal, ib.signal) and (ia.weight is None) == (ib.weight is None) and (ia.weight is None or torch.equal(ia.weight, ib.weight))
    a, b = left_out.run().data, spelled.run().data
    assert set(left_out.products) == set(spelled.products)
    assert set(left_out.products) == {"data", "weight", "blocks", "rhs", "residuals", "n_iter", "converged"} | ({"filter_aware", "preprocessing"} if filter_aware else set())
    assert np.array_equal(np.isnan(a), np.isnan(b))
    for key in ("weight", "blocks", "rhs"):
        v, w = left_out.products[key], spelled.products[key]
        assert np.abs(v - w).max() <= 1e-12 * np.abs(v).max(), key
    ok = np.isfinite(a)
    if filter_aware:
        assert left_out.products["n_iter"] == spelled.products["n_iter"] and left_out.products["converged"] and spelled.products["converged"]
        assert np.abs(a[ok] - b[ok]).max() <= 1e-6 * np.abs(a[ok]).max()
    else:
        assert np.array_equal(bits(a), bits(b))
