"""mrx_tod_column_fit, mrx_tod_column_apply, maria_amd.sky_polynomial and TOD.remove_sky_polynomial on the device (DESIGN
3.36), against the numpy float64 reference of tests/skypoly_ref.py.

hits is exact.  On small integers with a dyadic basis every float64 sum is exact in any order: N and r are compared bit for
bit.  On Gaussian data a sum of n terms is within (n + 1) 2^-53 sum|terms| of math.fsum, the correctly rounded sum of the
same rounded terms (Higham 2002, (4.4): n - 1 roundings of at most 2^-53 each on partial sums no larger than sum|terms|,
and fsum's own).  The verdict is regress.solve's on the device's own N and r; the coefficients are compared with a
longdouble solve of the device's own N and r through err / (2^-53 cond_2(M) |c|), M the scaled matrix.  The application is
compared bit for bit: its float64 steps and its one float32 operation are the reference's own."""

import numpy as np
import pytest
import skypoly_ref as ref
from test_gpu_flagging import device_rows, untouched_outside

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = [1, 2, 3, 4, 5, 6, 7, 9, 63, 65, 257]
LENGTHS = [1, 2, 3, 5, 63, 64, 65, 255, 257, 511, 513, 1023, 1025, 2051, 4099]
GROUPS = [1, 3, 16]
U = 2.0**-53
# err / (2^-53 cond_2(M) |c|) of the device's coefficients against a longdouble solve of the device's own sums: twice the
# largest value measured on an MI355X (5.73 over the 18 cases of test_the_solve).  Higham's bound for a
# Cholesky solve, 4 K (3 K + 1), is 16 at K = 1 and 456 at K = 6
RATIO_MAX = 11.5
# TOD.remove_sky_polynomial against the reference on host copies, in float32 ulps of the subtracted value: twice the largest
# value measured on an MI355X, which is 0 in every case: the outputs equal the reference's in every bit
K_ULPS = 0.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def dev(a):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run_fit(gpu_ctx, case, padded=False, with_model=True, with_off=True, min_hits=1, rcond=1e-10, columns=None, check_inputs=True):
    """(c, ok, hits, N, r) as host arrays of sky_polynomial.fit on the case (samples ``columns`` only: a slice)."""
    import torch

    from maria_amd import sky_polynomial as sp

    x, model, flags = case["x"], case["model"], case["flags"]
    if columns is not None:
        x, model, flags = x[:, columns], model[:, columns], None if flags is None else flags[:, columns]
    T = x.shape[1]
    pads = ((T + 3, 1), (T + 5, 3), (T + 1, 1)) if padded else ((T, 0),) * 3
    xbuf, xv = device_rows(x, *pads[0], -3.0)
    mbuf, mv = device_rows(model, *pads[1], -5.0)
    fbuf, fv = device_rows(flags, *pads[2], 9) if flags is not None else (None, None)
    bufs = [b for b in (xbuf, mbuf, fbuf) if b is not None]
    before = [b.clone() for b in bufs]
    G = case["n_groups"]
    D = x.shape[0]
    out = sp.fit(xv, dev(case["P"]), dev(case["u"]), dev(case["v"]), off=dev(case["off"]) if with_off else None,
                 groups=None if G == 1 and D < 3 else case["groups"], n_groups=G, flags=fv, model=mv if with_model else None,
                 min_hits=min_hits, rcond=rcond, sums=True, ctx=gpu_ctx)
    torch.cuda.synchronize()
    if check_inputs:
        assert all(torch.equal(a, b) or bool(((a == b) | (a != a)).all()) for a, b in zip(bufs, before)), "an input changed"
    c, ok, hits, N, r = out
    K = case["P"].shape[1]
    assert c.dtype == N.dtype == r.dtype == torch.float64 and ok.dtype == torch.bool and hits.dtype == torch.int64
    assert tuple(c.shape) == tuple(r.shape) == (G, K, T) and tuple(N.shape) == (G, K * (K + 1) // 2, T) and tuple(ok.shape) == tuple(hits.shape) == (G, T)
    return tuple(v.cpu().numpy() for v in out)


def reference_sums(case, with_model=True, with_off=True):
    G, D = case["n_groups"], case["x"].shape[0]
    groups = None if G == 1 and D < 3 else case["groups"]
    return ref.sums(case["x"], case["P"], case["u"], case["v"], off=case["off"] if with_off else None, groups=groups, n_groups=G,
                    flags=case["flags"], model=case["model"] if with_model else None)


def check_verdict(c, ok, hits, N, r, min_hits, where):
    """ok and c = 0 against the reference's solve of the device's own sums, wherever no pivot lies within a factor 1e3 of
    rcond (rank-deficient systems have pivots of rounding size, far below; the rest far above)."""
    G, K, T = c.shape
    for g in range(G):
        c_ref, ok_ref, piv = ref.solve(N[g], r[g], hits[g], min_hits=min_hits)
        with np.errstate(invalid="ignore"):
            clear = ~((piv > 1e-13) & (piv < 1e-7)).any(axis=0)
        assert np.array_equal(ok[g][clear], ok_ref[clear]), where
        assert not c[g][:, ~ok[g]].any(), where
        assert not ok[g][hits[g] < max(min_hits, K)].any(), where


def sums_case(gpu_ctx, D, T, G, K, variant, exact):
    seed = 1000 * T + 10 * D + G + 100 * K
    flag_rate, padded, with_model, with_off = variant
    case = ref.case(D, T, G, K, seed, exact, flag_rate=flag_rate)
    c, ok, hits, N, r = run_fit(gpu_ctx, case, padded=padded, with_model=with_model, with_off=with_off)
    N_ref, r_ref, h_ref, aN, ar = reference_sums(case, with_model, with_off)
    where = (D, T, G, K, variant, exact)
    np.testing.assert_array_equal(hits, h_ref, err_msg=str(where))
    if G >= 2:
        assert not h_ref[seed % G].any() and not ok[seed % G].any()  # the empty group
    if case["special"] is not None:
        g0, t0, tK, tK1 = case["special"]
        assert hits[g0, t0] == 0 and hits[g0, tK] == K and hits[g0, tK1] == K - 1 and not ok[g0, t0] and not ok[g0, tK1]
        assert not N[g0, :, t0].any() and not r[g0, :, t0].any()
    check_verdict(c, ok, hits, N, r, 1, where)
    if exact:
        assert np.array_equal(bits(N), bits(N_ref)) and np.array_equal(bits(r), bits(r_ref)), where  # bit for bit
        return 0.0
    worst = 0.0
    groups = np.zeros(D, np.int64) if G == 1 and D < 3 else case["groups"]
    picks = np.unique(np.concatenate([np.linspace(0, T - 1, min(T, 12)).astype(int), [s for s in (case["special"] or ())[1:]]]).astype(int))
    for g in range(G):
        if not (groups == g).any():
            continue
        N_x, r_x = ref.exact_sums(case["x"], case["P"], case["u"], case["v"], picks, g, off=case["off"] if with_off else None, groups=groups,
                                  flags=case["flags"], model=case["model"] if with_model else None)
        bN, br = (h_ref[g, picks] + 1) * U * aN[g][:, picks], (h_ref[g, picks] + 1) * U * ar[g][:, picks]
        assert np.all(np.abs(N[g][:, picks] - N_x) <= bN) and np.all(np.abs(r[g][:, picks] - r_x) <= br), where
        worst = max(worst, float((np.abs(r[g][:, picks] - r_x) / np.where(br > 0, br, 1)).max()))
    return worst


# (flag rate, padded pitches at odd element offsets, model, offsets)
VARIANTS = [(0.3, True, True, True), (0.0, False, False, False), (0.3, False, False, True), (0.0, True, True, False)]


def shapes(K):
    """Every length, with the rows, the group counts and the variants going round."""
    for i, T in enumerate(LENGTHS):
        yield ROWS[(i + 2 * K) % len(ROWS)], T, GROUPS[(i + K) % 3], VARIANTS[(i + K) % 4]
    for i, D in enumerate(ROWS):  # every row count, at lengths around a tile of K <= 4 and of K >= 5
        yield D, LENGTHS[(3 * i + K) % len(LENGTHS)], GROUPS[(i + K + 1) % 3], VARIANTS[(i + K + 2) % 4]


@pytest.mark.parametrize("K", range(1, 7))
def test_sums_are_exact_on_small_integers(gpu_ctx, K):
    for D, T, G, variant in shapes(K):
        sums_case(gpu_ctx, D, T, G, K, variant, exact=True)


@pytest.mark.parametrize("K", range(1, 7))
def test_sums_within_float64_rounding(gpu_ctx, K):
    worst = 0.0
    for D, T, G, variant in shapes(K):
        worst = max(worst, sums_case(gpu_ctx, D, T, G, K, variant, exact=False))
    print(f"K {K}: max |r - fsum| / ((n + 1) 2^-53 sum|terms|) = {worst:.3g}")


@pytest.mark.parametrize("with_flags", [False, True])
def test_one_term_is_the_column_mean(gpu_ctx, with_flags):
    """K = 1 with P = 1: N and r are bit for bit the W and S of mrx_tod_column_mean, on Gaussian data."""
    from maria_amd import regress

    for D, T, G in ((65, 4099, 3), (257, 1025, 1), (7, 513, 16)):
        case = ref.case(D, T, G, 1, D + T, exact=False, flag_rate=0.3 if with_flags else 0.0)
        assert np.all(case["P"][(case["groups"] >= 0) & (case["groups"] < G)] == 1.0)
        case["P"][:] = 1.0
        case["x"][case["v"] == 0] = 1.0  # the column mean reads these rows (and adds v = 0)
        u = np.where(case["v"] > 0, case["u"], 0.0)
        case["u"] = u
        c, ok, hits, N, r = run_fit(gpu_ctx, case)
        _, S, W = regress.column_mean(dev(case["x"]), dev(u), dev(case["v"]), off=dev(case["off"]), groups=case["groups"], n_groups=G,
                                      flags=dev(case["flags"]), model=dev(case["model"]), ctx=gpu_ctx)
        S, W = S.cpu().numpy(), W.cpu().numpy()
        # (a row with v = 0 adds u (x - off) = +-0 and v = 0 to the column mean: no bit of a sum that is not itself -0)
        assert np.array_equal(bits(N[:, 0] + 0.0), bits(W + 0.0)) and np.array_equal(bits(r[:, 0] + 0.0), bits(S + 0.0)), (D, T, G)


def test_the_same_bits_whatever_shares_the_call(gpu_ctx):
    """A second call; a slice of the samples alone; rows of other groups and of none put between the group's rows; wide
    and single accesses; 1e30 and NaN under the flags: the same bits.  An unflagged NaN stays in its own sample."""
    D, T, G = 65, 4099, 2
    for K in (1, 3, 4, 6):
        case = ref.case(D, T, G, K, 50 + K, exact=False)
        case["groups"] = np.where(case["groups"] >= 0, 0, -1).astype(np.int32)
        first = run_fit(gpu_ctx, case)
        again = run_fit(gpu_ctx, case)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)), K
        for lo, hi in ((0, 1), (1021, 2051), (4095, 4099)):  # other tiles, other positions in the thread's own samples
            part = run_fit(gpu_ctx, case, columns=slice(lo, hi))
            assert all(np.array_equal(bits(a[..., lo:hi]), bits(b)) for a, b in zip(first, part)), (K, lo, hi)
        odd = run_fit(gpu_ctx, case, padded=True)
        wide_out = run_fit(gpu_ctx, case, columns=slice(0, 4096))  # pitches of 4096 elements: 16-byte accesses
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, odd)), K
        assert all(np.array_equal(bits(a[..., :4096]), bits(b)) for a, b in zip(first, wide_out)), K
        # rows of another group and of none between the rows
        rng = np.random.default_rng(6)
        D2 = 3 * D
        place = np.sort(rng.choice(D2, D, replace=False))
        g2 = rng.choice([-1, 1], D2).astype(np.int32)
        g2[place] = case["groups"]

        def spread(a, fill):
            out = np.full((D2,) + a.shape[1:], fill, a.dtype)
            out[place] = a
            return out

        mixed = dict(x=spread(case["x"], 1e6), model=spread(case["model"], -1e6), flags=spread(case["flags"], 0), groups=g2,
                     P=spread(case["P"], 0.5), u=spread(case["u"], 7.0), v=spread(case["v"], 7.0), off=spread(case["off"], 7.0), n_groups=G)
        got = run_fit(gpu_ctx, mixed)
        assert all(np.array_equal(bits(a[0]), bits(b[0])) for a, b in zip(first, got)), K
        assert got[2][1].min() > 0  # the other group was summed too
        # what the flagged samples hold
        for fill in (1e30, np.nan):
            spoiled = dict(case, x=np.where(case["flags"] != 0, np.float32(fill), case["x"]))
            got = run_fit(gpu_ctx, spoiled)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, got)), (K, fill)
        # an unflagged NaN
        row = int(np.flatnonzero((case["groups"] == 0) & (case["v"] > 0))[2])
        t = int(np.flatnonzero(case["flags"][row] == 0)[5])
        x2 = case["x"].copy()
        x2[row, t] = np.nan
        c, ok, hits, N, r = run_fit(gpu_ctx, dict(case, x=x2))
        others = np.arange(T) != t
        assert np.isnan(r[0, :, t]).all() and np.array_equal(bits(N), bits(first[3])) and np.array_equal(ok, first[1])
        assert np.array_equal(bits(r[..., others]), bits(first[4][..., others])) and np.array_equal(bits(c[..., others]), bits(first[0][..., others]))


@pytest.mark.parametrize("K", [3, 6])
def test_past_the_first_trip_of_the_grid(gpu_ctx, K):
    """D = 7 and more (group, tile) items than the 8 n_cu workgroups of the launch (mrx_resident_blocks): 16 groups of
    R / 16 + 2 tiles of 1024 (K <= 4) or 512 (K >= 5, with flags) samples, the last one partial; the fit, and at K = 3 the
    application (its tile is 1024 samples at every K)."""
    import torch

    from maria_amd import sky_polynomial as sp

    R = 8 * int(gpu_ctx.device_info()["n_cu"])
    tile = 256 * (4 if K <= 4 else 2)
    G, D = 16, 7
    T = (R // G + 1) * tile + 5
    n_items = G * -(-T // tile)
    print(f"{n_items} work items, a grid of {R}")
    assert n_items > R
    rng = np.random.default_rng(K)
    x = rng.integers(-64, 65, (D, T)).astype(np.float32)
    flags = (rng.random((D, T)) < 0.3).astype(np.uint8)
    groups = np.array([15, 0, 15, 15, 7, 15, 0], np.int32)
    P = rng.integers(-4, 5, (D, K)) / 4.0
    P[:, 0] = 1.0
    u = rng.integers(1, 5, D).astype(np.float64)
    case = dict(x=x, model=np.zeros_like(x), flags=flags, groups=groups, P=P, u=u, v=u, off=np.zeros(D), n_groups=G)
    c, ok, hits, N, r = run_fit(gpu_ctx, case, with_model=False, with_off=False)
    N_ref, r_ref, h_ref, _, _ = ref.sums(x, P, u, u, groups=groups, n_groups=G, flags=flags)
    assert np.array_equal(hits, h_ref) and np.array_equal(bits(N), bits(N_ref)) and np.array_equal(bits(r), bits(r_ref))
    check_verdict(c, ok, hits, N, r, 1, K)
    cc = rng.integers(-8, 9, (G, K, T)).astype(np.float64)
    want = ref.apply(x, P, cc, u, groups=groups)
    got = sp.apply(dev(x), dev(P), dev(cc), dev(u), groups=groups, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_the_solve(gpu_ctx):
    """ok is regress.solve's verdict on the device's own N and r; c against a longdouble solve of them.  The inputs keep
    every pivot above 1e-3 or are rank-deficient by construction (test_host_skypoly.py checks both)."""
    from maria_amd import regress

    worst, same = 0.0, True
    for D, T, G in ref.SOLVE_CASES:
        for K in range(1, 7):
            case = ref.case(D, T, G, K, 100 * K + D, exact=False)
            for dup in (False, True):
                if dup and K < 2:
                    continue
                if dup:
                    case["P"][:, K - 1] = case["P"][:, 0 if K == 2 else 1]
                c, ok, hits, N, r = run_fit(gpu_ctx, case, min_hits=1)
                for g in range(G):
                    full = ref.full_matrices(N[g], K)
                    a_t, ok_t = regress.solve(dev(full), dev(r[g].T.copy()), dev(hits[g]), min_hits=1)
                    assert np.array_equal(ok[g], ok_t.cpu().numpy()), (D, T, G, K, dup, g)
                    assert np.array_equal(ok[g], hits[g] >= K) if not dup else not ok[g].any()
                    assert not c[g][:, ~ok[g]].any()
                    if dup or not ok[g].any():
                        continue
                    fit = ok[g]
                    c_ld, ok_ld, _ = ref.solve(N[g][:, fit], r[g][:, fit], hits[g][fit], min_hits=1, dtype=np.longdouble)
                    assert ok_ld.all()
                    M, _ = ref.scaled(N[g][:, fit], K)
                    kappa = np.linalg.cond(M)
                    err = np.sqrt(((c[g][:, fit].astype(np.longdouble) - c_ld) ** 2).sum(axis=0)).astype(np.float64)
                    size = np.sqrt((c_ld.astype(np.float64) ** 2).sum(axis=0))
                    ratio = err / (U * kappa * size)
                    worst = max(worst, float(ratio.max()))
                    assert ratio.max() <= 4 * K * (3 * K + 1), "above Higham's bound for Cholesky: a defect"
                    assert ratio.max() <= RATIO_MAX, (D, T, G, K, g, float(ratio.max()))
                    c_64 = ref.solve(N[g][:, fit], r[g][:, fit], hits[g][fit], min_hits=1)[0]
                    same = same and np.array_equal(bits(c_64), bits(c[g][:, fit]))
    print(f"max err / (2^-53 cond_2(M) |c|) = {worst:.3g}; the bits of the reference's float64 solve: {same}")


@pytest.mark.parametrize("K", [1, 3, 4, 6])
def test_application_bit_for_bit(gpu_ctx, K):
    import torch

    from maria_amd import sky_polynomial as sp

    G = 2
    for i, T in enumerate([1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099]):
        D = ROWS[(i + K) % len(ROWS)]
        rng = np.random.default_rng(T + D + K)
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        P = rng.uniform(-1, 1, (D, K))
        c = rng.standard_normal((G, K, T)) * 4
        h, e = rng.uniform(0.5, 2.0, D), rng.standard_normal(D)
        groups = rng.integers(-1, G, D).astype(np.int32)
        if D >= 2:
            groups[:2] = [-1, 1]
        dP, dc, dh, de = dev(P), dev(c), dev(h), dev(e)
        for pitch, offset in ((T + (-T) % 4, 0), (T, 0), (T + 3, 1)):
            for sign in (-1, 1):
                with_e = (sign + pitch) % 2 == 0
                want = ref.apply(x, P, c, h, e=e if with_e else None, groups=groups, sign=sign)
                assert np.array_equal(want[groups < 0], x[groups < 0])
                xbuf, xv = device_rows(x, pitch, offset, -3.0)
                before = xbuf.clone()
                ybuf, yv = device_rows(np.zeros_like(x), pitch + 4, offset, 7.0)
                yv.fill_(7.0)
                out = sp.apply(xv, dP, dc, dh, e=de if with_e else None, groups=groups, sign=sign, out=yv, ctx=gpu_ctx)
                torch.cuda.synchronize()
                assert out is yv and torch.equal(xbuf, before), "the input changed"
                assert np.array_equal(bits(yv.cpu().numpy()), bits(want)), (T, D, pitch, offset, sign)
                assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"
                out = sp.apply(xv, dP, dc, dh, e=de if with_e else None, groups=groups, sign=sign, out=xv, ctx=gpu_ctx)  # in place
                torch.cuda.synchronize()
                assert out is xv and np.array_equal(bits(xv.cpu().numpy()), bits(want)), (T, D, pitch, offset, sign, "in place")
                assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"
        got = sp.inject_gradient(dev(x), dP, dc, gains=dh, offsets=de, groups=groups, ctx=gpu_ctx)
        assert np.array_equal(got.cpu().numpy(), ref.apply(x, P, c, h, e=e, groups=groups, sign=+1))
        got = sp.apply(dev(x), dP, dc[:1].contiguous(), dh, ctx=gpu_ctx)  # groups=None, out=None, sign=-1
        assert np.array_equal(got.cpu().numpy(), ref.apply(x, P, c[:1], h))


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T, G, K = 4, 3000, 2, 3
    f64 = dict(dtype=torch.float64, device=DEV)
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    model = torch.zeros((D, T), dtype=torch.float32, device=DEV)
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    group = dev(np.array([0, 1, -1, 0], np.int32))
    P = dev(np.array([[1, 0.5, 0], [1, 0, 0], [1, 0, 0], [1, -0.5, 0.5]]))
    u = torch.ones(D, **f64)
    c = torch.full((G, K, T + 2), 7.0, **f64)
    ok = torch.full((G, T), 7, dtype=torch.uint8, device=DEV)
    hits = torch.full((G, T), 12345, dtype=torch.int32, device=DEV)
    N = torch.full((G, 6, T), 7.0, **f64)
    r = torch.full((G, K, T), 7.0, **f64)
    y = torch.full((D, T + 4), 7.0, dtype=torch.float32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    fit = (ptr(x), T, ptr(model), T, ptr(flags), T, D, T, ptr(group), G, ptr(P), K, ptr(u), ptr(u), ptr(u), 1, 1e-10, ptr(c), T + 2, ptr(ok),
           ptr(hits), ptr(N), ptr(r))
    ap = (ptr(x), T, D, T, ptr(group), G, ptr(P), K, ptr(c), T + 2, ptr(u), ptr(u), -1, ptr(y), T + 4)

    def put(args, *pairs):
        args = list(args)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    cases = {
        "mrx_tod_column_fit": {
            "null x": put(fit, (0, None)), "null P": put(fit, (10, None)), "null u": put(fit, (12, None)), "null v": put(fit, (13, None)),
            "null c": put(fit, (17, None)), "null ok": put(fit, (19, None)), "D 0": put(fit, (6, 0)), "T 0": put(fit, (7, 0)), "G 0": put(fit, (9, 0)),
            "G 17": put(fit, (9, 17)), "K 0": put(fit, (11, 0)), "K 7": put(fit, (11, 7)), "ld_x < T": put(fit, (1, T - 1)),
            "ld_m < T": put(fit, (3, T - 1)), "ld_f < T": put(fit, (5, T - 1)), "ld_c < T": put(fit, (18, T - 1)), "min_hits 0": put(fit, (15, 0)),
            "rcond 1": put(fit, (16, 1.0)), "rcond < 0": put(fit, (16, -1e-3)), "rcond nan": put(fit, (16, float("nan"))),
        },
        "mrx_tod_column_apply": {
            "null x": put(ap, (0, None)), "null P": put(ap, (6, None)), "null c": put(ap, (8, None)), "null h": put(ap, (11, None)),
            "null y": put(ap, (13, None)), "D 0": put(ap, (2, 0)), "T 0": put(ap, (3, 0)), "G 0": put(ap, (5, 0)), "G 17": put(ap, (5, 17)),
            "K 0": put(ap, (7, 0)), "K 7": put(ap, (7, 7)), "sign 0": put(ap, (12, 0)), "sign 2": put(ap, (12, 2)), "ld_x < T": put(ap, (1, T - 1)),
            "ld_y < T": put(ap, (14, T - 1)), "ld_c < T": put(ap, (9, T - 1)), "in place at another pitch": put(ap, (13, ptr(x)), (14, T + 4)),
        },
    }
    for entry, bad in cases.items():
        for name, args in bad.items():
            assert getattr(lib, entry)(hd, *args) == -1, (entry, name)
            assert entry.encode() in lib.mrx_last_error(hd), (entry, name)
    torch.cuda.synchronize()
    for out in (c, N, r, y):
        assert bool((out == 7.0).all())
    assert bool((ok == 7).all()) and bool((hits == 12345).all()) and bool((x == 1.0).all())
    # a pitch of an array that is not given is not looked at; model, flags, groups, offsets and the sums may be null
    assert lib.mrx_tod_column_fit(hd, *put(fit, (2, None), (3, 0), (4, None), (5, 0), (8, None), (14, None), (20, None), (21, None), (22, None))) == 0
    torch.cuda.synchronize()
    # all four rows in group 0, K = 3 on four rows of which two coincide: the third pivot is 1/2 ... a plain fit of x = 1
    assert bool((ok[0] == 1).all()) and bool((ok[1] == 0).all()) and bool((c[1, :, :T] == 0).all()) and bool((c[:, :, T:] == 7.0).all())
    assert bool((N == 7.0).all()) and bool((hits == 12345).all())
    assert lib.mrx_tod_column_fit(hd, *fit) == 0
    torch.cuda.synchronize()
    assert hits[:, 0].tolist() == [2, 1] and N[:, 0, 5].tolist() == [2.0, 1.0] and not bool(ok.any()) and not bool(c[:, :, :T].any())
    assert lib.mrx_tod_column_apply(hd, *ap) == 0  # c = 0: y = x - (float)(1 + 1 * 0)
    torch.cuda.synchronize()
    assert bool((y[:, :T] == torch.tensor([0.0, 0.0, 1.0, 0.0], device=DEV)[:, None]).all()) and bool((y[:, T:] == 7.0).all())
    assert lib.mrx_tod_column_apply(hd, *put(ap, (4, None), (10, None))) == 0  # no groups, no e: every row in group 0
    torch.cuda.synchronize()
    assert bool((y[:, :T] == 1.0).all()) and bool((y[:, T:] == 7.0).all())


@pytest.mark.parametrize("K", [3, 6])
def test_the_science_fixture(gpu_ctx, K):
    """61 detectors on a hexagonal lattice, white noise of sigma 1 under gains, offsets, 5 % flags and random-walk
    coefficients of amplitude 20 on K terms (tests/skypoly_ref.py: science): fitted with the injected gains and offsets,
    the matching order leaves sigma sqrt(1 - K / (0.95 D)) +- 3 % over the unflagged samples, the order below more than
    4 sigma.  (test_host_skypoly.py has the same in numpy, within 0.5 %.)"""
    from maria_amd import sky_polynomial as sp

    x, flags, pos, gains, offs, c, _ = ref.science(K)
    D = len(pos)
    dx, df = dev(x), dev(flags)
    for order, matching in (({3: 0, 6: 1}[K], False), ({3: 1, 6: 2}[K], True)):
        P = sp.basis(pos, order)
        k = P.shape[1]
        cc, ok, _, _, _ = sp.fit(dx, dev(P), dev(gains), dev(gains * gains), off=dev(offs), flags=df, min_hits=2 * k, ctx=gpu_ctx)
        assert bool(ok.all())
        y = sp.apply(dx, dev(P), cc, dev(gains), e=dev(offs), ctx=gpu_ctx).cpu().numpy()
        rms = ref.residual_rms(y, flags)
        print(f"injected K {K}, fitted K {k}: residual {rms:.4f} sigma; expected for a matching order {np.sqrt(1 - k / (0.95 * D)):.4f}")
        if matching:
            assert abs(rms / np.sqrt(1 - k / (0.95 * D)) - 1) <= 0.03
        else:
            assert rms > 4.0
    # the whole chain, gains and offsets fitted: every sample fitted, the residual printed (DESIGN 3.36 says why it is larger)
    P = dev(sp.basis(pos, {3: 1, 6: 2}[K]))
    cc, ok_t, g, o, ok_d = sp.fit_sky(dx, P, flags=df, ctx=gpu_ctx)
    assert bool(ok_t.all()) and bool(ok_d.all())
    y = sp.apply(dx, P, cc, g, e=o, ctx=gpu_ctx).cpu().numpy()
    print(f"fit_sky, gains from fit_common_mode: residual {ref.residual_rms(y, flags):.4f} sigma")


def host(v):
    import torch

    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def ulps_of_the_subtracted(got, want, x):
    """max over samples of |got - want| in float32 ulps of the row's largest subtracted value (x - want)."""
    sub = np.abs(x.astype(np.float64) - want.astype(np.float64)).max(axis=1)
    ulp = np.spacing(np.maximum(sub, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp[:, None]).max())


@pytest.fixture(scope="module")
def atmosphere_tod(gpu_ctx):
    import torch
    from test_gpu_regress import simulated

    tod = simulated()
    tod.data = {"atmosphere": torch.as_tensor(tod.data["atmosphere"]).to(DEV, torch.float32)}
    assert tuple(tod.data["atmosphere"].shape) == (64, 3000) and sorted(set(tod.dets.band_index.tolist())) == [0, 1]
    return tod


TOD_CASES = {
    "plane": dict(), "constant": dict(order=0), "quadratic": dict(order=2), "one group": dict(groups=None, order=2), "model": dict(model=True),
    "into": dict(into="extra"), "left out": dict(groups="some"), "not flagged": dict(flag_failed=False, min_dets=31),
}


@pytest.mark.parametrize("case", list(TOD_CASES))
@pytest.mark.parametrize("chain", ["plain", "flagged and downsampled"])
def test_tod_remove_sky_polynomial_against_the_reference(gpu_ctx, atmosphere_tod, case, chain):
    """TOD.remove_sky_polynomial on a simulated atmosphere against skypoly_ref.remove on host copies of the same float32
    signal: within K_ULPS float32 ulps of the subtracted value; the metadata; the failed samples and their flags."""
    import torch

    from maria_amd import sky_polynomial as sp
    from maria_amd.sim import TOD

    src = atmosphere_tod
    kw = dict(TOD_CASES[case])
    data = {"atmosphere": src.data["atmosphere"].clone()}
    if kw.get("into") == "extra" or kw.get("model"):
        rng = np.random.default_rng(3)
        data["extra"] = (0.01 * rng.standard_normal(tuple(src.data["atmosphere"].shape))).astype(np.float32)  # a host field
    tod = TOD(data, src.dets, src.coords, units=src.units, metadata=dict(src.metadata))
    tod._calibrator = getattr(src, "_calibrator", None)
    if chain != "plain":
        tod = tod.flag_glitches(n_sigma=3.0, ctx=gpu_ctx).downsample(4, ctx=gpu_ctx)
        assert tod.flags is not None and 0 < float((tod.flags != 0).float().mean()) < 0.5
    D, T = tod.data["atmosphere"].shape
    band = np.asarray(tod.dets.band_index, np.int32)
    if kw.get("groups", "band") == "some":
        kw["groups"] = np.where(np.arange(D) % 7 == 3, -1, band).astype(np.int32)
    if kw.get("model"):
        kw["model"] = tod.data["extra"]
    if case == "not flagged":  # a sample that 31 of a band's 32 detectors cannot fit: one flag more than min_dets allows
        few = torch.zeros((D, T), dtype=torch.uint8, device=DEV) if tod.flags is None else tod.flags.clone()
        few[np.flatnonzero(band == 1)[:2].tolist(), 17] = 1
        tod.flags = few
    kept = {k: host(v).copy() for k, v in tod.data.items()}
    out = tod.remove_sky_polynomial(ctx=gpu_ctx, **kw)
    assert "sky_polynomial" not in tod.metadata and all(np.array_equal(host(tod.data[k]), v) for k, v in kept.items())
    assert out.fields == tod.fields and out.dets is tod.dets and out.coords is tod.coords and out.units == tod.units
    assert out._calibrator is getattr(tod, "_calibrator", None)
    for v in out.data.values():
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (D, T)
    # the reference on the host, from the same float32 signal
    signal = sum(kept.values()).astype(np.float32) if len(kept) > 1 else kept["atmosphere"]
    groups = band if case not in ("one group", "left out") else (None if case == "one group" else kw["groups"])
    G = 1 if groups is None else 2
    order = kw.get("order", 1)
    K = ref.n_terms(order)
    P = ref.basis(tod.dets.offsets, order, groups, G)
    np.testing.assert_allclose(P, sp.basis(tod.dets.offsets, order, groups, G), rtol=0, atol=4e-16)
    P = sp.basis(tod.dets.offsets, order, groups, G)
    flags = None if tod.flags is None else host(tod.flags)
    model = None if kw.get("model") is None else kept["extra"]
    into = kw.get("into", "atmosphere")
    min_dets = kw.get("min_dets", 2 * K)
    want, c, ok_t, g, o, ok_d = ref.remove(signal, kept[into], P, groups=groups, n_groups=G, flags=flags, model=model, min_dets=min_dets)
    got = host(out.data[into])
    for name in kept:
        if name != into:
            assert np.array_equal(host(out.data[name]), kept[name]), name
    grouped = np.ones(D, bool) if groups is None else groups >= 0
    assert ok_d.tolist() == grouped.tolist() and np.array_equal(got[~grouped], kept[into][~grouped])
    meta = out.metadata["sky_polynomial"]
    assert meta["order"] == order and meta["n_terms"] == K and meta["n_groups"] == G and meta["n_iter"] == 3 and meta["min_dets"] == min_dets
    assert meta["coefficients"].dtype == np.float64 and meta["coefficients"].shape == (G, K, T) and meta["gains"].shape == meta["offsets"].shape == (D,)
    assert meta["failed_rows"].size == 0 and meta["flag_failed"] == kw.get("flag_failed", True)
    assert np.array_equal(meta["failed_samples"], np.argwhere(~ok_t))
    gr = np.zeros(D, np.int64) if groups is None else np.asarray(groups, np.int64)
    failed = ~ok_t[np.where(grouped, gr, 0)] & grouped[:, None]
    if case == "not flagged":
        assert [1, 17] in meta["failed_samples"].tolist() and out.flags is tod.flags
        rows = np.flatnonzero(band == 1)  # only the offset is taken from a sample that is not fitted
        assert np.array_equal(got[rows, 17], (kept[into][rows, 17] - o[rows].astype(np.float32)))
    else:
        new_flags = np.zeros((D, T), np.uint8) if out.flags is None else host(out.flags)
        assert np.array_equal(new_flags != 0, failed | (False if flags is None else flags != 0))
    k = ulps_of_the_subtracted(got, want, kept[into])
    fit = ok_t.any(axis=1)
    c_err = float(np.abs(meta["coefficients"] - c).max() / np.abs(c).max())
    gain_err = float(np.abs(meta["gains"] - g)[grouped].max())
    before = np.sqrt(((signal - signal.mean(axis=1, keepdims=True)) ** 2).mean(axis=1))
    after_signal = sum(host(v) for v in out.data.values())
    after = np.sqrt(((after_signal - after_signal.mean(axis=1, keepdims=True)) ** 2).mean(axis=1))
    print(f"{case}, {chain}: {k:.3f} float32 ulps of the subtracted value; max |c - ref| / max|c| {c_err:.2e}; max |gain - ref| {gain_err:.2e}; "
          f"samples not fitted {int((~ok_t).sum())}; largest row rms after / before {float((after[grouped] / before[grouped]).max()):.3e}")
    assert fit.all() and k <= K_ULPS
    assert gain_err <= 1e-6 and c_err <= 1e-6  # parts in 1e12: the order of a few float64 sums of fit_common_mode and its solver
    assert np.all(after[grouped] < before[grouped])


def test_the_map_of_the_cleaned_tod(gpu_ctx):
    """BinMapper of TOD.remove_sky_polynomial's result against BinMapper of the reference-cleaned TOD.  A pixel is a weighted
    mean of samples, so two TODs within K_ULPS ulps of the subtracted value give pixels within that; the binner adds its
    float64 sums with atomics, in an order that changes from run to run: 2 n 2^-53 max|sample| a run for at most n = D T
    samples in a pixel (Higham 2002, (4.4), for the sum and for the weight).  The float64 maps are compared under the sum of
    the two.  Against the input map the plane leaves less than the raw TOD."""
    import torch
    from test_gpu_regress import simulated

    from maria_amd import sky_polynomial as sp
    from maria_amd.mappers import BinMapper
    from maria_amd.sim import TOD

    tod, sky, centre, bands, n, res = simulated(with_map=True)
    cleaned = tod.remove_sky_polynomial(order=1, into="atmosphere", ctx=gpu_ctx)
    kept = {k: host(v).astype(np.float32) for k, v in tod.data.items()}
    signal = sum(kept.values()).astype(np.float32)
    D, T = signal.shape
    band = np.asarray(tod.dets.band_index, np.int32)
    want, *_ = ref.remove(signal, kept["atmosphere"], sp.basis(tod.dets.offsets, 1, band, 2), groups=band, n_groups=2)
    k_tod = ulps_of_the_subtracted(host(cleaned.data["atmosphere"]), want, kept["atmosphere"])
    assert k_tod <= K_ULPS
    data = {k: (torch.as_tensor(want).to(DEV) if k == "atmosphere" else v) for k, v in tod.data.items()}
    by_ref = TOD(data, tod.dets, tod.coords, units=tod.units, metadata=dict(tod.metadata), flags=cleaned.flags)
    by_ref._calibrator = getattr(tod, "_calibrator", None)
    maps, residual = {}, {}
    for name, t in (("raw", tod), ("cleaned", cleaned), ("reference", by_ref)):
        mapper = BinMapper([t], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="I", nu=[b.center for b in bands],
                           frame="ra/dec", units="K_RJ")
        out = mapper.run()
        maps[name] = np.asarray(mapper.products["data"][0], np.float64)
        w = mapper.products["weight"][0, -1]
        residual[name] = np.sqrt(np.nansum(w * (np.asarray(out.data[0, :]) - sky.data[0, 0]) ** 2, axis=(-1, -2)) / np.nansum(w))
    both = np.isfinite(maps["cleaned"]) & np.isfinite(maps["reference"])
    assert np.array_equal(np.isfinite(maps["cleaned"]), np.isfinite(maps["reference"])) and both.mean() > 0.2
    sub = float(np.abs(kept["atmosphere"].astype(np.float64) - want).max())
    top = float(np.abs(want.astype(np.float64) + sum(v for k, v in kept.items() if k != "atmosphere")).max())  # the largest binned sample
    bound = K_ULPS * float(np.spacing(np.float32(sub))) + 4 * D * T * U * top
    diff = float(np.abs(maps["cleaned"][both] - maps["reference"][both]).max())
    print(f"map of the cleaned TOD against the reference's: max |difference| {diff:.3e} K_RJ, {diff / bound:.3e} of the bound {bound:.3e}; "
          f"TOD {k_tod:.3f} ulps; weighted rms residual per band [K_RJ]: raw {residual['raw']}, plane removed {residual['cleaned']}")
    assert diff <= bound
    assert np.all(residual["cleaned"] < residual["raw"])
