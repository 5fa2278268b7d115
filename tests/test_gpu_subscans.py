"""mrx_tod_segment_normal, mrx_tod_segment_apply, maria_amd.subscans and TOD.filter_subscans on the device,
against the numpy float64 reference of tests/subscans_ref.py.

The reference's sums are math.fsum over the rounded products, so a device sum of a segment of L samples may differ from it
by the worst case of any float64 summation order, L 2^-53 sum|terms| to first order, plus fsum's own half ulp: the bound is
(L + 1) 2^-53 sum|terms|.  Where a sum is exact in any order (small integers at K = 1) or is a single product (one kept
sample) it is compared bit for bit, which pins the basis to the bit.  The application is compared bit for bit: its float64
steps and its one float32 operation are the reference's own."""

import numpy as np
import pytest
import subscans_ref as ref
from test_gpu_downsample import _centre
from test_gpu_flagging import device_rows, untouched_outside
from test_host_subscans import SCAN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = [1, 3, 33]
TIMES = [1, 5, 255, 256, 257, 1023, 1024, 1025, 4099]
LENGTHS = [0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1024, 1025, 2049]
HALF_ULP = 2.0**-53


def make_bounds(T, seed):
    """[S + 1] int32: the LENGTHS in a random order from sample min(2, T // 3) on, as many as fit before the last
    min(3, T // 3) samples: some samples in no segment at both ends (from T = 3)."""
    rng = np.random.default_rng(seed)
    b = [min(2, T // 3)]
    for L in rng.permutation(LENGTHS):
        if b[-1] + L <= T - min(3, T // 3):
            b.append(b[-1] + int(L))
    return np.array(b, np.int32)


def test_the_bounds_of_the_cases_hold_every_length():
    used = set()
    for K in range(1, 9):
        for T in TIMES:
            b = make_bounds(T, 10 * K + T)
            assert len(b) >= 2 and b[0] >= 0 and b[-1] <= T and (T < 3 or (b[0] > 0 and b[-1] < T))
            used |= set(np.diff(b).tolist())
    assert used == set(LENGTHS)


def rows(D, T, seed, exact):
    """(x, model, flags): small integers (exact sums) or Gaussian; flags random at 10 %, values 1 and 2."""
    rng = np.random.default_rng(seed)
    if exact:
        x = rng.integers(-64, 65, (D, T)).astype(np.float32)
        model = rng.integers(-16, 17, (D, T)).astype(np.float32)
    else:
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        model = rng.standard_normal((D, T)).astype(np.float32)
    flags = ((rng.random((D, T)) < 0.1) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    return x, model, flags


def to_device(x, model, flags, padded):
    """Padded pitches in buffers that start one (x, flags) or three (model) elements off alignment, or plain tensors."""
    T = x.shape[1]
    pads = ((T + 3, 1), (T + 5, 3), (T + 1, 1)) if padded else ((T, 0),) * 3
    bufs = device_rows(x, *pads[0], -3.0), device_rows(model, *pads[1], -5.0), device_rows(flags, *pads[2], 9)
    return [b for b, _ in bufs], [v for _, v in bufs]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def normal_case(gpu_ctx, D, T, K, with_flags, with_model, padded, exact):
    import torch

    from maria_amd import subscans

    seed = 1000 * T + 10 * D + K
    bounds = make_bounds(T, 10 * K + T)
    x, model, flags = rows(D, T, seed, exact)
    if T >= 64:
        lo, hi = bounds[1], bounds[2]
        flags[D - 1, lo:hi] = 2  # one segment wholly flagged in the last row
    bufs, (xv, mv, fv) = to_device(x, model, flags, padded)
    before = [b.clone() for b in bufs]
    N, r, hits = subscans.normal_equations(xv, bounds, K, flags=fv if with_flags else None, model=mv if with_model else None, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"
    S = len(bounds) - 1
    assert N.dtype == r.dtype == torch.float64 and hits.dtype == torch.int64
    assert tuple(N.shape) == (D, S, K, K) and tuple(r.shape) == (D, S, K) and tuple(hits.shape) == (D, S)
    N_ref, r_ref, h_ref, aN, ar = ref.normal_equations(x, bounds, K, flags=flags if with_flags else None, model=model if with_model else None)
    where = (D, T, K, with_flags, with_model, padded)
    N_got, r_got = N.cpu().numpy(), r.cpu().numpy()
    np.testing.assert_array_equal(hits.cpu().numpy(), h_ref, err_msg=str(where))  # exact everywhere
    assert np.array_equal(N_got, N_got.transpose(0, 1, 3, 2)), where
    empty = np.diff(bounds) == 0
    assert not N_got[:, empty].any() and not r_got[:, empty].any() and not h_ref[:, empty].any()
    if exact:
        assert np.array_equal(bits(N_got), bits(N_ref)) and np.array_equal(bits(r_got), bits(r_ref)), where
        return 0.0
    L = np.diff(bounds).astype(np.float64)
    bN, br = (L[None, :, None, None] + 1) * HALF_ULP * aN, (L[None, :, None] + 1) * HALF_ULP * ar
    assert np.all(np.abs(N_got - N_ref) <= bN) and np.all(np.abs(r_got - r_ref) <= br), where
    return float(max((np.abs(r_got - r_ref) / np.where(br > 0, br, 1)).max(), (np.abs(N_got - N_ref) / np.where(bN > 0, bN, 1)).max()))


@pytest.mark.parametrize("D", ROWS)
def test_one_polynomial_on_small_integers_bit_for_bit(gpu_ctx, D):
    """K = 1: N = hits and r = the sum of integers below 2^7 less integers below 2^5, exact in any order."""
    for i, T in enumerate(TIMES):
        normal_case(gpu_ctx, D, T, 1, with_flags=True, with_model=i % 2 == 0, padded=i % 2 == 1, exact=True)
        normal_case(gpu_ctx, D, T, 1, with_flags=i % 2 == 1, with_model=True, padded=i % 2 == 0, exact=True)


@pytest.mark.parametrize("K", range(1, 9))
def test_sums_within_float64_rounding_and_hits_exact(gpu_ctx, K):
    worst = 0.0
    for i, T in enumerate(TIMES):
        D = ROWS[(i + K) % 3]
        worst = max(worst, normal_case(gpu_ctx, D, T, K, with_flags=True, with_model=True, padded=(i + K) % 2 == 0, exact=False))
        if T in (5, 257, 1025):
            worst = max(worst, normal_case(gpu_ctx, ROWS[(i + K + 1) % 3], T, K, with_flags=False, with_model=False, padded=(i + K) % 2 == 1, exact=False))
    print(f"K {K}: max |sum - ref| / ((L + 1) 2^-53 sum|terms|) = {worst:.3g}")


@pytest.mark.parametrize("K", range(1, 9))
def test_one_kept_sample_pins_the_basis(gpu_ctx, K):
    """Segments of 2 .. 65 samples side by side, row p with every sample flagged but position p of each segment (none
    where the segment is shorter): N and r are single products, P_i P_j and P_i term at that position, bit for bit."""
    import torch

    from maria_amd import subscans

    lengths = np.arange(2, 66)
    bounds = np.concatenate([[2], 2 + np.cumsum(lengths)]).astype(np.int32)
    D, T = 65, int(bounds[-1]) + 3
    x, model, _ = rows(D, T, 77 + K, exact=False)
    flags = np.ones((D, T), np.uint8)
    N_ref, r_ref, h_ref = np.zeros((D, 64, K, K)), np.zeros((D, 64, K)), np.zeros((D, 64), np.int64)
    for s, L in enumerate(lengths):
        P = ref.basis(int(L), K)
        p = np.arange(L)
        t = bounds[s] + p
        flags[p, t] = 0
        term = x[p, t].astype(np.float64) - model[p, t].astype(np.float64)
        N_ref[p, s] = (P[:, None, :] * P[None, :, :]).transpose(2, 0, 1)
        r_ref[p, s] = (P * term[None, :]).T
        h_ref[p, s] = 1
    N_ref, r_ref = N_ref + 0.0, r_ref + 0.0  # a sum that starts at +0 never ends at -0
    for padded in (False, True):
        _, (xv, mv, fv) = to_device(x, model, flags, padded)
        N, r, hits = subscans.normal_equations(xv, bounds, K, flags=fv, model=mv, ctx=gpu_ctx)
        assert torch.equal(hits.cpu(), torch.as_tensor(h_ref))
        assert np.array_equal(bits(N.cpu().numpy()), bits(N_ref)) and np.array_equal(bits(r.cpu().numpy()), bits(r_ref)), (K, padded)


def test_sums_are_reproducible_alone_and_at_either_alignment(gpu_ctx):
    """The same bits on a second call, for a row alone, for a segment alone (its own two bounds), with or without the
    other arguments' company, and at either alignment: the order is a function of the segment's ends alone."""
    import torch

    from maria_amd import subscans

    D, T = 33, 4099
    x, model, flags = rows(D, T, 8, exact=False)
    dx, dm, df = (torch.as_tensor(a).to(DEV) for a in (x, model, flags))
    for K in (1, 4, 5, 8):
        bounds = make_bounds(T, K)
        S = len(bounds) - 1
        first = subscans.normal_equations(dx, bounds, K, flags=df, model=dm, ctx=gpu_ctx)
        again = subscans.normal_equations(dx, bounds, K, flags=df, model=dm, ctx=gpu_ctx)
        for a, c in zip(first, again):
            assert np.array_equal(bits(a.cpu().numpy()), bits(c.cpu().numpy()))
        for row in (0, 16, 32):
            alone = subscans.normal_equations(dx[row:row + 1], bounds, K, flags=df[row:row + 1], model=dm[row:row + 1], ctx=gpu_ctx)
            for a, c in zip(first, alone):
                assert np.array_equal(bits(a[row:row + 1].cpu().numpy()), bits(c.cpu().numpy())), (K, row)
        for s in range(S):
            alone = subscans.normal_equations(dx, bounds[s:s + 2], K, flags=df, model=dm, ctx=gpu_ctx)
            for a, c in zip(first, alone):
                assert np.array_equal(bits(a[:, s:s + 1].cpu().numpy()), bits(c.cpu().numpy())), (K, s)
        wide = [device_rows(v, 4100, 0, 0)[1] for v in (x, model, flags)]
        odd = [device_rows(v, 4101, 1, 0)[1] for v in (x, model, flags)]
        for layout in (wide, odd):
            got = subscans.normal_equations(layout[0], bounds, K, flags=layout[2], model=layout[1], ctx=gpu_ctx)
            for a, c in zip(first, got):
                assert np.array_equal(bits(a.cpu().numpy()), bits(c.cpu().numpy())), K
        # the sums of the first polynomials do not depend on how many follow them
        if K > 1:
            fewer = subscans.normal_equations(dx, bounds, K - 1, flags=df, model=dm, ctx=gpu_ctx)
            assert torch.equal(fewer[0], first[0][:, :, :K - 1, :K - 1]) and torch.equal(fewer[1], first[1][:, :, :K - 1])


def test_hostile_bounds_are_clamped(gpu_ctx):
    """The C entries with bounds below 0, above T and reversed: clamped, a reversed pair empty, nothing out of range."""
    import torch

    from maria_amd import subscans
    from maria_amd._lib import ptr

    D, T, K = 3, 300, 4
    x, model, flags = rows(D, T, 21, exact=False)
    bufs, (xv, mv, fv) = to_device(x, model, flags, True)
    before = [b.clone() for b in bufs]
    raw = np.array([-2**31, -7, 5, 3, 3, 140, 120, T + 9, 2**31 - 1], np.int32)  # [0, 0) [0, 5) [5, 3) [3, 3) [3, 140) [140, 120) [120, 300) [300, 300)
    S = len(raw) - 1
    assert [hi - lo for lo, hi in ref.segments(raw, T)] == [0, 5, -2, 0, 137, -20, 180, 0]
    d_raw = torch.as_tensor(raw).to(DEV)
    N = torch.full((D, S, K, K), 7.0, dtype=torch.float64, device=DEV)
    r = torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV)
    hits = torch.full((D, S), 12345, dtype=torch.int32, device=DEV)
    gpu_ctx.call("mrx_tod_segment_normal", ptr(xv), T + 3, ptr(mv), T + 5, ptr(fv), T + 1, D, T, ptr(d_raw), S, K, ptr(N), ptr(r), ptr(hits))
    torch.cuda.synchronize()
    N_ref, r_ref, h_ref, aN, ar = ref.normal_equations(x, raw, K, flags=flags, model=model)
    assert np.array_equal(hits.cpu().numpy(), h_ref) and h_ref[:, [0, 2, 3, 5, 7]].sum() == 0 and h_ref[:, [1, 4, 6]].all()
    assert np.all(np.abs(N.cpu().numpy() - N_ref) <= 301 * HALF_ULP * aN) and np.all(np.abs(r.cpu().numpy() - r_ref) <= 301 * HALF_ULP * ar)
    # the application through the Python side, whose bounds ascend: clamped at both ends, every sample covered
    asc = np.array([-7, 5, 5, 140, T + 9], np.int32)
    a = np.random.default_rng(22).standard_normal((D, 4, K))
    want = ref.apply(x, asc, a, sign=+1)
    ybuf, yv = device_rows(np.zeros_like(x), T + 7, 1, 7.0)
    subscans.apply(xv, asc, torch.as_tensor(a).to(DEV), sign=+1, out=yv, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert np.array_equal(bits(yv.cpu().numpy()), bits(want)) and not np.array_equal(want, x)
    assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"
    # reversed bounds in the application: whichever segment a sample is given to, nothing is written outside the rows
    ybuf, yv = device_rows(np.zeros_like(x), T + 7, 1, 7.0)
    a8 = torch.zeros((D, S, K), dtype=torch.float64, device=DEV)
    gpu_ctx.call("mrx_tod_segment_apply", ptr(xv), T + 3, D, T, ptr(d_raw), S, K, ptr(a8), -1, ptr(yv), T + 7)
    torch.cuda.synchronize()
    assert np.array_equal(yv.cpu().numpy(), x) and untouched_outside(ybuf, yv, 7.0)  # a = 0: a copy
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"


@pytest.mark.parametrize("K", [1, 2, 4, 5, 8])
def test_application_bit_for_bit(gpu_ctx, K):
    import torch

    from maria_amd import subscans

    for i, T in enumerate(TIMES):
        D = ROWS[(i + K) % 3]
        rng = np.random.default_rng(T + D + K)
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        bounds = make_bounds(T, 10 * K + T)
        S = len(bounds) - 1
        a = rng.standard_normal((D, S, K))
        da = torch.as_tensor(a).to(DEV)
        covered = np.zeros(T, bool)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            covered[lo:hi] = True
        assert T < 3 or not covered[[0, -1]].any()
        # 16-byte accesses: a pitch that is a multiple of four words; single words: the row pitch T, and T + 3 one word in
        for pitch, offset in ((T + (-T) % 4, 0), (T, 0), (T + 3, 1)):
            for sign in (-1, 1):
                want = ref.apply(x, bounds, a, sign=sign)
                assert np.array_equal(want[:, ~covered], x[:, ~covered])
                xbuf, xv = device_rows(x, pitch, offset, -3.0)
                before = xbuf.clone()
                ybuf, yv = device_rows(np.zeros_like(x), pitch + 4, offset, 7.0)
                yv.fill_(7.0)
                out = subscans.apply(xv, bounds, da, sign=sign, out=yv, ctx=gpu_ctx)
                torch.cuda.synchronize()
                assert out is yv and torch.equal(xbuf, before), "the input changed"
                assert np.array_equal(bits(yv.cpu().numpy()), bits(want)), (T, D, pitch, offset, sign)
                assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"
                out = subscans.apply(xv, bounds, da, sign=sign, out=xv, ctx=gpu_ctx)  # in place
                torch.cuda.synchronize()
                assert out is xv and np.array_equal(bits(xv.cpu().numpy()), bits(want)), (T, D, pitch, offset, sign, "in place")
                assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"
        dx = torch.as_tensor(x).to(DEV)
        assert np.array_equal(subscans.apply(dx, bounds, da, ctx=gpu_ctx).cpu().numpy(), ref.apply(x, bounds, a, sign=-1))  # out=None, sign=-1
        assert np.array_equal(subscans.inject_drifts(dx, bounds, da, ctx=gpu_ctx).cpu().numpy(), ref.apply(x, bounds, a, sign=+1))


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T, S, K = 4, 3000, 3, 3
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    model = torch.zeros((D, T), dtype=torch.float32, device=DEV)
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    bound = torch.as_tensor(np.array([0, 1000, 1000, T], np.int32)).to(DEV)
    a = torch.ones((D, S, K), dtype=torch.float64, device=DEV)
    N = torch.full((D, S, K, K), 7.0, dtype=torch.float64, device=DEV)
    r = torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV)
    hits = torch.full((D, S), 12345, dtype=torch.int32, device=DEV)
    y = torch.full((D, T + 4), 7.0, dtype=torch.float32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    ne = (ptr(x), T, ptr(model), T, ptr(flags), T, D, T, ptr(bound), S, K, ptr(N), ptr(r), ptr(hits))
    ap = (ptr(x), T, D, T, ptr(bound), S, K, ptr(a), -1, ptr(y), T + 4)

    def put(args, *pairs):
        args = list(args)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    cases = {
        "mrx_tod_segment_normal": {
            "null x": put(ne, (0, None)), "null bound": put(ne, (8, None)), "null N": put(ne, (11, None)), "null r": put(ne, (12, None)),
            "D 0": put(ne, (6, 0)), "T 0": put(ne, (7, 0)), "S 0": put(ne, (9, 0)), "S -1": put(ne, (9, -1)), "K 0": put(ne, (10, 0)),
            "K 9": put(ne, (10, 9)), "ld_x < T": put(ne, (1, T - 1)), "ld_m < T": put(ne, (3, T - 1)), "ld_f < T": put(ne, (5, T - 1)),
        },
        "mrx_tod_segment_apply": {
            "null x": put(ap, (0, None)), "null bound": put(ap, (4, None)), "null a": put(ap, (7, None)), "null y": put(ap, (9, None)),
            "D 0": put(ap, (2, 0)), "T 0": put(ap, (3, 0)), "S 0": put(ap, (5, 0)), "K 0": put(ap, (6, 0)), "K 9": put(ap, (6, 9)),
            "sign 0": put(ap, (8, 0)), "sign 2": put(ap, (8, 2)), "ld_x < T": put(ap, (1, T - 1)), "ld_y < T": put(ap, (10, T - 1)),
            "in place at another pitch": put(ap, (9, ptr(x)), (10, T + 4)),
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
    assert lib.mrx_tod_segment_normal(hd, *put(ne, (2, None), (3, 0), (4, None), (5, 0), (13, None))) == 0
    torch.cuda.synchronize()
    assert N[:, :, 0, 0].tolist() == [[1000.0, 0.0, 2000.0]] * D and r[:, :, 0].tolist() == [[1000.0, 0.0, 2000.0]] * D and bool((hits == 12345).all())
    assert lib.mrx_tod_segment_normal(hd, *ne) == 0 and lib.mrx_tod_segment_apply(hd, *ap) == 0
    torch.cuda.synchronize()
    assert hits.tolist() == [[1000, 0, 2000]] * D and not bool(N[:, 1].any())
    # y = 1 - (P_0 + P_1 + P_2)(u): 1 - 3 at u = +1, the last sample, and 1 - (1 - 1 + 1) at u = -1, the first
    assert y[:, T - 1].tolist() == [-2.0] * D and y[:, 0].tolist() == [0.0] * D and bool((y[:, T:] == 7.0).all())


def test_flagged_samples_do_not_touch_the_fit(gpu_ctx):
    """Random flags: what the flagged samples hold (the data, 1e30, NaN) changes no bit of a, of ok, or of any unflagged
    sample of the result."""
    import torch

    from maria_amd import subscans

    D, T, K = 33, 4099, 6
    x, model, flags = rows(D, T, 31, exact=False)
    bounds = make_bounds(T, 3)
    flags[7, :] = 1
    dm, df = torch.as_tensor(model).to(DEV), torch.as_tensor(flags).to(DEV)
    results = []
    for fill in (None, 1e30, float("nan")):
        xx = torch.as_tensor(x).to(DEV)
        if fill is not None:
            xx[df != 0] = fill
        a, ok = subscans.fit(xx, bounds, K, flags=df, model=dm, ctx=gpu_ctx)
        y = subscans.apply(xx, bounds, a, ctx=gpu_ctx)
        results.append((a.cpu().numpy(), ok.cpu().numpy(), y.cpu().numpy()[flags == 0]))
    ok = results[0][1]
    assert not ok[7].any() and ok[0].sum() >= 6 and np.isfinite(results[0][0]).all()
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(bits(a), bits(b))


def scan_tod(x, flags=None):
    """A TOD of the [D, 3000] device tensor ``x`` on the front-end test's scan (tests/test_host_subscans.py: SCAN)."""
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates, Plan

    plan = Plan.back_and_forth(start_time=1.7e9, scan_center=(120.0, 55.0), **SCAN)
    D = x.shape[0]
    dets = Detectors(np.zeros((D, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int))
    return TOD({"signal": x}, dets, Coordinates(plan.time, plan.phi, plan.theta), units="K_RJ", flags=flags)


@pytest.mark.parametrize("order", [0, 3, 7])
def test_injected_drifts_are_taken_out(gpu_ctx, order):
    """Polynomials of degree <= order, different in every (detector, segment), injected into zeros: filter_subscans leaves
    |residual| <= 8 * 2^-24 max|x| of the row on the fitted segments (the bound of test_gpu_regress.py::
    test_an_injected_common_mode_is_taken_out_exactly: the injection, the rounded fit and the subtraction, a rounding
    each, and a factor to spare; the float64 reference reaches 1.05 * 2^-24 on such input); the segments that cannot be
    fitted are bit-identical to the input, listed in the metadata and flagged whole."""
    import torch

    from maria_amd import subscans

    D, T, K = 33, 3000, order + 1
    tod0 = scan_tod(torch.zeros((D, T), dtype=torch.float32, device=DEV))
    bounds, turn = subscans.find_subscans(tod0.coords._baz)
    S = len(bounds) - 1
    assert S == 13 and bounds[-1] - bounds[-2] == 25
    rng = np.random.default_rng(40 + order)
    coeffs = rng.uniform(-1, 1, (D, S, K)) * rng.uniform(0.1, 10.0, (D, 1, 1))
    x = subscans.inject_drifts(tod0.data["signal"], bounds, torch.as_tensor(coeffs).to(DEV), ctx=gpu_ctx)
    old = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    old[2, bounds[3]:bounds[4] - 5] = 2  # a second segment that cannot be fitted: 5 samples left, all in the turnaround
    old[:, 100:110] = 1
    tod = scan_tod(x, flags=old)
    out = tod.filter_subscans(order=order, ctx=gpu_ctx)
    assert "subscans" not in tod.metadata and torch.equal(tod.data["signal"], x) and out.dets is tod.dets and out.coords is tod.coords
    assert out.units == tod.units and out._calibrator is getattr(tod, "_calibrator", None)
    meta = out.metadata["subscans"]
    assert meta["order"] == order and meta["bounds"].tolist() == bounds.tolist() and meta["turn_frac"] == 0.9 and meta["min_hits"] == 8
    assert meta["rcond"] == 1e-10 and meta["coefficients"].shape == (D, S, K)
    failed = np.zeros((D, S), bool)
    failed[:, S - 1] = True  # 25 samples, all but the last two or three in the turnaround
    failed[2, 3] = True
    assert sorted(map(tuple, meta["failed_segments"].tolist())) == sorted(map(tuple, np.argwhere(failed).tolist()))
    y, xh, fl = out.data["signal"].cpu().numpy(), x.cpu().numpy(), out.flags.cpu().numpy()
    top = np.abs(xh).max(axis=1)
    worst = 0.0
    want_flags = old.cpu().numpy() | turn[None, :]
    for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        for d in range(D):
            if failed[d, s]:
                assert np.array_equal(bits(y[d, lo:hi]), bits(xh[d, lo:hi])) and fl[d, lo:hi].all() and not meta["coefficients"][d, s].any()
                want_flags[d, lo:hi] |= 1
            else:
                worst = max(worst, float(np.abs(y[d, lo:hi]).max() / (2.0**-24 * top[d])))
    print(f"order {order}: max |residual| / (2^-24 max|x|) on the fitted segments = {worst:.3f}")
    assert worst <= 8.0
    assert np.array_equal(fl != 0, want_flags != 0)
    # the flags' switches
    plain = tod.filter_subscans(order=order, flag_turnarounds=False, flag_failed=False, ctx=gpu_ctx)
    assert torch.equal(plain.flags, old) and torch.equal(plain.data["signal"], out.data["signal"])
    only_failed = tod.filter_subscans(order=order, flag_turnarounds=False, ctx=gpu_ctx).flags.cpu().numpy()
    assert np.array_equal(only_failed != 0, (old.cpu().numpy() != 0) | np.repeat(failed, np.diff(bounds), axis=1))
    # bounds of one's own: two segments a crossing, the coefficients of the halves differ from the whole's
    halves = np.sort(np.concatenate([bounds, (bounds[:-1] + bounds[1:]) // 2])).astype(np.int32)
    own = tod.filter_subscans(order=order, bounds=halves, ctx=gpu_ctx)
    assert own.metadata["subscans"]["coefficients"].shape == (D, 2 * S, K) and own.metadata["subscans"]["bounds"].tolist() == halves.tolist()


@pytest.fixture(scope="module")
def scanned_atmosphere(gpu_ctx):
    """Simulation(atmosphere="2d") of 32 positions x 2 bands (test_gpu_regress.py's configuration) on the constant-elevation
    scan, 50 Hz, K_RJ."""
    import torch

    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation

    bands = [Band(center=93e9, width=27e9, shape="top_hat", name="f093"), Band(center=150e9, width=41e9, shape="top_hat", name="f150")]
    inst = Instrument(Detectors.hexagon(32, 0.5, bands, primary_size=30.0))
    plan = Plan.back_and_forth(start_time=1.7e9, scan_center=(120.0, 55.0), **SCAN)
    (tod,) = Simulation(inst, plan, Site(altitude=5000.0), atmosphere="2d", atmosphere_kwargs={"n_layers": 2, "seed": 4, "pwv_rms_frac": 0.1},
                        noise=False).run()
    assert tod.units == "K_RJ" and tod.fields == ["atmosphere"]
    tod.data = {"atmosphere": torch.as_tensor(tod.data["atmosphere"]).to(DEV, torch.float32)}
    assert tuple(tod.data["atmosphere"].shape) == (64, 3000)
    return tod


@pytest.mark.parametrize("case", ["plain", "flagged, order 5", "model, into another field"])
def test_tod_filter_subscans_against_the_reference(gpu_ctx, scanned_atmosphere, case):
    """TOD.filter_subscans on a simulated atmosphere under the constant-elevation scan against subscans_ref.
    filter_subscans on the same float32 signal on the host: every sample within 2^-22 max(max|x|, max|fit|) of its row (one
    float32 rounding of the fit and one of the difference, where the two fits differ by float64 roundings only); the
    flags and the unfitted segments are the reference's; every fitted row's rms falls."""
    import torch

    from maria_amd import subscans
    from maria_amd.sim import TOD

    src = scanned_atmosphere
    D, T = 64, 3000
    data = {"atmosphere": src.data["atmosphere"].clone()}
    kw, flags = dict(order=3), None
    if case == "flagged, order 5":
        kw = dict(order=5)
        flags = (np.random.default_rng(5).random((D, T)) < 0.05).astype(np.uint8) * 2
    if case == "model, into another field":
        data["extra"] = (0.01 * np.random.default_rng(3).standard_normal((D, T))).astype(np.float32)  # a host field
        kw = dict(order=3, model=data["extra"], into="extra")
    tod = TOD(data, src.dets, src.coords, units=src.units, metadata=dict(src.metadata), flags=None if flags is None else torch.as_tensor(flags).to(DEV))
    tod._calibrator = getattr(src, "_calibrator", None)
    kept = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v).copy() for k, v in tod.data.items()}
    out = tod.filter_subscans(ctx=gpu_ctx, **kw)
    assert out.fields == tod.fields and out._calibrator is tod._calibrator and out.dets is tod.dets and out.coords is tod.coords
    for v in out.data.values():
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (D, T)
    bounds, turn = subscans.find_subscans(src.coords._baz)
    assert len(bounds) - 1 == 13 and abs(turn.mean() - 0.18) < 0.01
    signal = sum(kept.values()).astype(np.float32) if len(kept) > 1 else kept["atmosphere"]
    into = kw.get("into", "atmosphere")
    y_ref, f_ref, a_ref, ok_ref = ref.filter_subscans(signal, kept[into], bounds, turn, kw["order"], flags=flags, model=kw.get("model"))
    assert ok_ref[:, :-1].all() and not ok_ref[:, -1].any()
    meta = out.metadata["subscans"]
    assert meta["failed_segments"].tolist() == [[d, 12] for d in range(D)] and np.array_equal(out.flags.cpu().numpy() != 0, f_ref != 0)
    got = out.data[into].cpu().numpy()
    for name in kept:
        if name != into:
            assert np.array_equal(out.data[name].cpu().numpy(), kept[name]), name
    assert np.array_equal(bits(got[:, bounds[-2]:]), bits(kept[into][:, bounds[-2]:]))  # the unfitted segment
    fit = ref.fit_values(bounds, a_ref, T)
    scale = np.maximum(np.abs(kept[into]).max(axis=1), np.abs(fit).max(axis=1))
    err = np.abs(got.astype(np.float64) - y_ref.astype(np.float64)).max(axis=1) / (2.0**-22 * scale)
    coef = np.abs(meta["coefficients"] - a_ref).max() / np.abs(a_ref).max()
    fitted = slice(0, bounds[-2])
    after = sum(v.cpu().numpy() for v in out.data.values())
    if kw.get("model") is not None:
        signal, after = signal - kw["model"], after - kw["model"]
    ratio = float((after[:, fitted].std(axis=1) / signal[:, fitted].std(axis=1)).max())
    print(f"{case}: max |y - ref| / (2^-22 max(max|x|, max|fit|)) = {err.max():.3f}; max |a - ref| / max|a| = {coef:.2e}; "
          f"largest row rms after / before {ratio:.3e}")
    assert np.all(err <= 1.0)
    assert ratio < 1.0


def test_the_map_through_drifts(gpu_ctx):
    """A ProjectionMap source sampled on the constant-elevation scan, polynomial drifts of order 3 injected per (detector,
    subscan) as a second field, filter_subscans(model=the sampled sky): BinMapper of the result equals BinMapper of the
    drift-free TOD with the same flags within 8 * 2^-24 max|x|, the bound of the TOD (test_injected_drifts_are_taken_out);
    a binned pixel is a mean of its samples, so the bound carries over."""
    import torch

    from maria_amd import map as mmap
    from maria_amd import subscans
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
    assert clean.units == "K_RJ" and set(clean.fields) == {"map"}
    sky_field = torch.as_tensor(clean.data["map"]).to(DEV, torch.float32)
    D, T = sky_field.shape
    assert (D, T) == (64, 3000) and float(sky_field.abs().max()) > 1e-3
    bounds, turn = subscans.find_subscans(clean.coords._baz)
    S = len(bounds) - 1
    assert S >= 20 and 0.1 < turn.mean() < 0.5
    rng = np.random.default_rng(9)
    coeffs = 0.05 * rng.uniform(-1, 1, (D, S, 4))
    drift = subscans.inject_drifts(torch.zeros_like(sky_field), bounds, torch.as_tensor(coeffs).to(DEV), ctx=gpu_ctx)
    dirty = TOD({"map": sky_field, "drift": drift}, clean.dets, clean.coords, units="K_RJ", metadata=dict(clean.metadata))
    cleaned = dirty.filter_subscans(order=3, model=dirty.data["map"], into="drift", ctx=gpu_ctx)
    assert torch.equal(cleaned.data["map"], sky_field) and cleaned.flags is not None
    free = TOD({"map": sky_field}, clean.dets, clean.coords, units="K_RJ", metadata=dict(clean.metadata), flags=cleaned.flags)
    maps = {}
    for name, tod in (("dirty", dirty), ("cleaned", cleaned), ("free", free)):
        mapper = BinMapper([tod], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="I",
                           nu=[b.center for b in bands], frame="ra/dec", units="K_RJ")
        maps[name] = np.asarray(mapper.run().data[0, :], np.float64)
        assert (mapper.products["weight"][0, -1] > 0).mean() > 0.05
    top = float((sky_field + drift).abs().max())
    assert np.array_equal(np.isnan(maps["cleaned"]), np.isnan(maps["free"]))
    hit = ~np.isnan(maps["free"])
    err = float(np.abs(maps["cleaned"] - maps["free"])[hit].max())
    raw = float(np.nanmax(np.abs(maps["dirty"] - maps["free"])))
    print(f"max |map(filtered) - map(drift-free)| = {err:.3e} K_RJ = {err / (2.0**-24 * top):.3f} x 2^-24 max|x|; with the drifts left in {raw:.3e} K_RJ")
    assert raw > 1e-3  # without this the test shows nothing
    assert err <= 8 * 2.0**-24 * top
