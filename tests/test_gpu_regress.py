"""mrx_tod_column_mean, mrx_tod_regress_normal, mrx_tod_regress_apply, maria_amd.regress, TOD.regress and
TOD.remove_common_mode on the device, against the numpy float64 reference of tests/regress_ref.py.

On small integers every float64 sum is exact in any order: S, W, mean, N, r and hits are compared bit for bit.  On Gaussian
data a sum of n terms may differ from the reference by the worst case of any float64 summation order, n 2^-52 sum|terms|,
and the mean, rounded once to float32, by 2^-23 |q| plus the bounds of S and W carried through the quotient.  The
application is compared bit for bit: its float64 steps and its one float32 operation are the reference's own."""

import numpy as np
import pytest
import regress_ref as ref
from test_gpu_downsample import _centre
from test_gpu_flagging import device_rows, untouched_outside
from test_host_regress import templates

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = [1, 2, 63, 64, 65, 1023, 1025, 4099]
ROWS = [1, 2, 3, 5, 63, 64, 65, 257]
EPS = 2.0**-52
# TOD front end against the reference, in float32 ulps of the subtracted combination: twice the largest value measured on
# an MI355X, which is 0 in all 22 cases: the outputs equal the reference's in every bit
K_ULPS = 0.0


def make_groups(D, G, seed):
    """[D] int32 in random row order: about a tenth of the rows -1 (from D = 3), and with G >= 2 one group empty."""
    rng = np.random.default_rng(seed)
    used = [g for g in range(G) if G == 1 or g != seed % G]
    groups = rng.choice(used, D).astype(np.int32)
    if D >= 3:
        groups[rng.random(D) < 0.1] = -1
        groups[rng.integers(0, D)] = -1
    return groups


def rows(D, T, seed, exact):
    """(x, model, flags, u, v, off): small integers (exact sums) or Gaussian; flags random at 3 %, values 1 and 2."""
    rng = np.random.default_rng(seed)
    if exact:
        x = rng.integers(-64, 65, (D, T)).astype(np.float32)
        model = rng.integers(-16, 17, (D, T)).astype(np.float32)
        u, v, off = (rng.integers(lo, 5, D).astype(np.float64) for lo in (-4, 0, -4))
    else:
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        model = rng.standard_normal((D, T)).astype(np.float32)
        u, v, off = rng.standard_normal(D), rng.uniform(0.5, 2.0, D), rng.standard_normal(D)
    flags = ((rng.random((D, T)) < 0.03) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    return x, model, flags, u, v, off


def special_flags(flags, groups, G, seed):
    """One row wholly flagged, and one sample flagged in every row of one group."""
    D, T = flags.shape
    flags[D - 1, :] = 2
    inside = groups[(groups >= 0) & (groups < G)]
    if inside.size:
        flags[groups == inside[0], seed % T] = 1
    return flags


# (flags, model, offsets, padded pitches at odd element offsets)
VARIANTS = [(True, True, True, True), (False, False, False, False), (True, False, True, False), (False, True, False, True)]


def to_device(x, model, flags, padded):
    T = x.shape[1]
    pads = ((T + 3, 1), (T + 5, 3), (T + 1, 1)) if padded else ((T, 0),) * 3
    bufs = device_rows(x, *pads[0], -3.0), device_rows(model, *pads[1], -5.0), device_rows(flags, *pads[2], 9)
    return [b for b, _ in bufs], [v for _, v in bufs]


def mean_case(gpu_ctx, D, T, G, variant, exact):
    import torch

    from maria_amd import regress

    with_flags, with_model, with_off, padded = variant
    seed = 1000 * T + 10 * D + G
    groups = make_groups(D, G, seed)
    x, model, flags, u, v, off = rows(D, T, seed + 1, exact)
    flags = special_flags(flags, groups, G, seed)
    bufs, (xv, mv, fv) = to_device(x, model, flags, padded)
    before = [b.clone() for b in bufs]
    du, dv, doff = (torch.as_tensor(a).to(DEV) for a in (u, v, off))
    kw = dict(groups=None if G == 1 and D < 3 else groups, n_groups=G)
    mean, S, W = regress.column_mean(xv, du, dv, off=doff if with_off else None, flags=fv if with_flags else None,
                                     model=mv if with_model else None, ctx=gpu_ctx, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"
    assert mean.dtype == torch.float32 and S.dtype == W.dtype == torch.float64 and tuple(mean.shape) == tuple(S.shape) == tuple(W.shape) == (G, T)
    S_ref, W_ref, m_ref, A_ref = ref.column_mean(x, u, v, off=off if with_off else None, flags=flags if with_flags else None,
                                                 model=model if with_model else None, **kw)
    where = (D, T, G, variant)
    if G >= 2:
        assert not W_ref[seed % G].any()  # the empty group
    S_got, W_got, m_got = S.cpu().numpy(), W.cpu().numpy(), mean.cpu().numpy()
    if exact:
        assert np.array_equal(S_got.view(np.uint64), S_ref.view(np.uint64)), where  # bit for bit
        assert np.array_equal(W_got.view(np.uint64), W_ref.view(np.uint64)), where
        assert np.array_equal(m_got.view(np.uint32), m_ref.view(np.uint32)), where
        return 0.0
    bS, bW = D * EPS * A_ref, D * EPS * W_ref
    assert np.all(np.abs(S_got - S_ref) <= bS) and np.all(np.abs(W_got - W_ref) <= bW), where
    ok = W_ref > 0
    q = np.where(ok, S_ref / np.where(ok, W_ref, 1), 0.0)
    carried = (bS + np.abs(q) * bW) / np.where(ok, W_ref - bW, 1)
    assert np.all(np.abs(m_got.astype(np.float64) - q) <= 2.0**-23 * np.abs(q) + carried), where
    assert not m_got[~ok].any()
    return float((np.abs(S_got - S_ref) / np.where(bS > 0, bS, 1)).max())


@pytest.mark.parametrize("D", ROWS)
def test_column_mean_is_exact_on_small_integers(gpu_ctx, D):
    for i, T in enumerate(LENGTHS):
        for G in (1, 2, 3):
            mean_case(gpu_ctx, D, T, G, VARIANTS[(i + G) % 4], exact=True)
            mean_case(gpu_ctx, D, T, G, VARIANTS[(i + G + 1) % 4], exact=True)


@pytest.mark.parametrize("D", ROWS)
def test_column_mean_within_float64_rounding(gpu_ctx, D):
    worst = 0.0
    for i, T in enumerate(LENGTHS):
        for G in (1, 2, 3):
            worst = max(worst, mean_case(gpu_ctx, D, T, G, VARIANTS[(i + G) % 2], exact=False))
    print(f"D {D}: max |S - ref| / (D 2^-52 sum|terms|) = {worst:.3g}")


def test_column_mean_is_reproducible_and_other_rows_do_not_enter(gpu_ctx):
    """The same bits on a second call, and the same bits for a group when rows of another group and of none are put
    between its rows."""
    import torch

    from maria_amd import regress

    D, T, G = 65, 4099, 2
    x, model, flags, u, v, off = rows(D, T, 5, exact=False)
    groups = np.zeros(D, np.int32)
    dx, dm, df, du, dv, doff = (torch.as_tensor(a).to(DEV) for a in (x, model, flags, u, v, off))
    first = regress.column_mean(dx, du, dv, off=doff, groups=groups, n_groups=G, flags=df, model=dm, ctx=gpu_ctx)
    again = regress.column_mean(dx, du, dv, off=doff, groups=groups, n_groups=G, flags=df, model=dm, ctx=gpu_ctx)
    for a, c in zip(first, again):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), c.cpu().numpy().view(np.uint8))
    rng = np.random.default_rng(6)
    D2 = 3 * D
    place = np.sort(rng.choice(D2, D, replace=False))  # where the group's rows go, in their order
    g2 = rng.choice([-1, 1], D2).astype(np.int32)
    g2[place] = 0

    def spread(a, fill):
        out = np.full((D2,) + a.shape[1:], fill, a.dtype)
        out[place] = a
        return torch.as_tensor(out).to(DEV)

    mixed = regress.column_mean(spread(x, 1e6), spread(u, 7.0), spread(v, 7.0), off=spread(off, 7.0), groups=g2, n_groups=G,
                                flags=spread(flags, 0), model=spread(model, -1e6), ctx=gpu_ctx)
    for a, c in zip(first, mixed):
        assert np.array_equal(a[0].cpu().numpy().view(np.uint8), c[0].cpu().numpy().view(np.uint8))
    assert float(mixed[2][1].min()) > 0  # the other group was summed too


def normal_case(gpu_ctx, D, T, G, K, variant, exact):
    import torch

    from maria_amd import regress

    with_flags, with_model, _, padded = variant
    seed = 1000 * T + 10 * D + G + 100 * K
    groups = make_groups(D, G, seed)
    x, model, flags, _, _, _ = rows(D, T, seed + 1, exact)
    flags = special_flags(flags, groups, G, seed)
    B = np.random.default_rng(seed + 2).integers(-4, 5, (G, K, T)).astype(np.float32) if exact else templates(G, K, T, seed + 2)
    bufs, (xv, mv, fv) = to_device(x, model, flags, padded)
    bbuf, bv = device_rows(B.reshape(G * K, T), T + 7 if padded else T, 1 if padded else 0, -7.0)
    bv = bv.unflatten(0, (G, K))
    bufs.append(bbuf)
    before = [b.clone() for b in bufs]
    kw = dict(groups=None if G == 1 and D < 3 else groups)
    N, r, hits = regress.normal_equations(xv, bv, flags=fv if with_flags else None, model=mv if with_model else None, ctx=gpu_ctx, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "an input changed"
    assert N.dtype == r.dtype == torch.float64 and hits.dtype == torch.int64
    assert tuple(N.shape) == (D, K, K) and tuple(r.shape) == (D, K) and tuple(hits.shape) == (D,)
    N_ref, r_ref, h_ref, aN, ar = ref.normal_equations(x, B, flags=flags if with_flags else None, model=model if with_model else None, **kw)
    where = (D, T, G, K, variant)
    N_got, r_got = N.cpu().numpy(), r.cpu().numpy()
    np.testing.assert_array_equal(hits.cpu().numpy(), h_ref, err_msg=str(where))
    assert np.array_equal(N_got, N_got.transpose(0, 2, 1)), where
    if with_flags and groups[D - 1] >= 0:
        assert h_ref[D - 1] == 0 and not N_got[D - 1].any() and not r_got[D - 1].any()
    if exact:
        assert np.array_equal(N_got.view(np.uint64), N_ref.view(np.uint64)), where  # bit for bit
        assert np.array_equal(r_got.view(np.uint64), r_ref.view(np.uint64)), where
        return 0.0
    bN, br = h_ref[:, None, None] * EPS * aN, h_ref[:, None] * EPS * ar
    assert np.all(np.abs(N_got - N_ref) <= bN) and np.all(np.abs(r_got - r_ref) <= br), where
    return float((np.abs(r_got - r_ref) / np.where(br > 0, br, 1)).max())


@pytest.mark.parametrize("K", range(1, 9))
def test_normal_equations_are_exact_on_small_integers(gpu_ctx, K):
    for i, T in enumerate(LENGTHS):
        for j in range(3):
            D, G = ROWS[(i + 3 * j + K) % 8], 1 + (i + j) % 3
            normal_case(gpu_ctx, D, T, G, K, VARIANTS[(i + j) % 4], exact=True)


@pytest.mark.parametrize("K", range(1, 9))
def test_normal_equations_within_float64_rounding(gpu_ctx, K):
    worst = 0.0
    for i, T in enumerate(LENGTHS):
        for j in range(2):
            D, G = ROWS[(i + 3 * j + K + 1) % 8], 1 + (i + j + 1) % 3
            worst = max(worst, normal_case(gpu_ctx, D, T, G, K, VARIANTS[(i + j) % 4], exact=False))
    print(f"K {K}: max |r - ref| / (n 2^-52 sum|terms|) = {worst:.3g}")


def test_normal_equations_are_reproducible_and_rows_do_not_see_each_other(gpu_ctx):
    import torch

    from maria_amd import regress

    D, T, G = 65, 4099, 2
    x, model, flags, _, _, _ = rows(D, T, 8, exact=False)
    groups = make_groups(D, G, 1)  # group 1 is the empty one
    groups[[0, 31, 64]] = 0
    dx, dm, df = (torch.as_tensor(a).to(DEV) for a in (x, model, flags))
    for K in (2, 3, 8):  # one of each compiled class
        host_B = templates(G, K, T, 9)
        B = torch.as_tensor(host_B).to(DEV)
        first = regress.normal_equations(dx, B, groups=groups, flags=df, model=dm, ctx=gpu_ctx)
        again = regress.normal_equations(dx, B, groups=groups, flags=df, model=dm, ctx=gpu_ctx)
        for a, c in zip(first, again):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), c.cpu().numpy().view(np.uint8))
        for row in (0, 31, 64):
            alone = regress.normal_equations(dx[row:row + 1], B, groups=groups[row:row + 1], flags=df[row:row + 1], model=dm[row:row + 1], ctx=gpu_ctx)
            for a, c in zip(first, alone):
                assert np.array_equal(a[row:row + 1].cpu().numpy().view(np.uint8), c.cpu().numpy().view(np.uint8)), (K, row)
        # 16-byte accesses (pitches of 4100 words) and single ones (4101 words, one word in): the order is a function of T alone
        wide = [device_rows(v, 4100, 0, 0)[1] for v in (x, model, flags, host_B.reshape(G * K, T))]
        odd = [device_rows(v, 4101, 1, 0)[1] for v in (x, model, flags, host_B.reshape(G * K, T))]
        for layout in (wide, odd):
            got = regress.normal_equations(layout[0], layout[3].unflatten(0, (G, K)), groups=groups, flags=layout[2], model=layout[1], ctx=gpu_ctx)
            for a, c in zip(first, got):
                assert np.array_equal(a.cpu().numpy().view(np.uint8), c.cpu().numpy().view(np.uint8)), K
        # the sums of the first templates do not depend on how many follow them (the K class)
        fewer = regress.normal_equations(dx, B[:, :1].contiguous(), groups=groups, flags=df, model=dm, ctx=gpu_ctx)
        assert torch.equal(fewer[0][:, 0, 0], first[0][:, 0, 0]) and torch.equal(fewer[1][:, 0], first[1][:, 0])


@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_application_bit_for_bit(gpu_ctx, K):
    import torch

    from maria_amd import regress

    G = 2
    for i, T in enumerate([1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099]):
        D = ROWS[(i + K) % 8]
        rng = np.random.default_rng(T + D + K)
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        B = rng.standard_normal((G, K, T)).astype(np.float32)
        a = rng.standard_normal((D, K))
        groups = rng.integers(-1, G, D).astype(np.int32)
        if D >= 2:
            groups[:2] = [-1, 1]
        da = torch.as_tensor(a).to(DEV)
        # 16-byte accesses: a pitch that is a multiple of four words; single words: the row pitch T, and T + 3 one word in
        for pitch, offset in ((T + (-T) % 4, 0), (T, 0), (T + 3, 1)):
            bbuf, bv = device_rows(B.reshape(G * K, T), pitch, offset, -7.0)
            bv = bv.unflatten(0, (G, K))
            for sign in (-1, 1):
                want = ref.apply(x, B, a, groups=groups, sign=sign)
                assert np.array_equal(want[groups < 0], x[groups < 0])
                xbuf, xv = device_rows(x, pitch, offset, -3.0)
                before = xbuf.clone()
                ybuf, yv = device_rows(np.zeros_like(x), pitch + 4, offset, 7.0)
                yv.fill_(7.0)
                out = regress.apply(xv, bv, da, groups=groups, sign=sign, out=yv, ctx=gpu_ctx)
                torch.cuda.synchronize()
                assert out is yv and torch.equal(xbuf, before), "the input changed"
                assert np.array_equal(yv.cpu().numpy().view(np.uint32), want.view(np.uint32)), (T, D, pitch, offset, sign)
                assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"
                out = regress.apply(xv, bv, da, groups=groups, sign=sign, out=xv, ctx=gpu_ctx)  # in place
                torch.cuda.synchronize()
                assert out is xv and np.array_equal(xv.cpu().numpy().view(np.uint32), want.view(np.uint32)), (T, D, pitch, offset, sign, "in place")
                assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"
        got = regress.apply(torch.as_tensor(x).to(DEV), torch.as_tensor(B).to(DEV), da, groups=groups, ctx=gpu_ctx)  # out=None, sign=-1
        assert np.array_equal(got.cpu().numpy(), ref.apply(x, B, a, groups=groups, sign=-1))


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T, G, K = 4, 3000, 2, 3
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    model = torch.zeros((D, T), dtype=torch.float32, device=DEV)
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    group = torch.as_tensor(np.array([0, 1, -1, 0], np.int32)).to(DEV)
    u = torch.ones(D, dtype=torch.float64, device=DEV)
    B = torch.ones((G, K, T), dtype=torch.float32, device=DEV)
    a = torch.ones((D, K), dtype=torch.float64, device=DEV)
    S = torch.full((G, T), 7.0, dtype=torch.float64, device=DEV)
    W = torch.full((G, T), 7.0, dtype=torch.float64, device=DEV)
    mean = torch.full((G, T), 7.0, dtype=torch.float32, device=DEV)
    N = torch.full((D, K, K), 7.0, dtype=torch.float64, device=DEV)
    r = torch.full((D, K), 7.0, dtype=torch.float64, device=DEV)
    hits = torch.full((D,), 12345, dtype=torch.int32, device=DEV)
    y = torch.full((D, T + 4), 7.0, dtype=torch.float32, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    cm = (ptr(x), T, ptr(model), T, ptr(flags), T, D, T, ptr(group), G, ptr(u), ptr(u), ptr(u), ptr(S), ptr(W), ptr(mean), T)
    ne = (ptr(x), T, ptr(model), T, ptr(flags), T, D, T, ptr(group), G, ptr(B), T, K, ptr(N), ptr(r), ptr(hits))
    ap = (ptr(x), T, D, T, ptr(group), G, ptr(B), T, K, ptr(a), -1, ptr(y), T + 4)

    def put(args, *pairs):
        args = list(args)
        for i, v in pairs:
            args[i] = v
        return tuple(args)

    cases = {
        "mrx_tod_column_mean": {
            "null x": put(cm, (0, None)), "null u": put(cm, (10, None)), "null v": put(cm, (11, None)),
            "no output": put(cm, (13, None), (14, None), (15, None)), "D 0": put(cm, (6, 0)), "T 0": put(cm, (7, 0)), "G 0": put(cm, (9, 0)),
            "G 17": put(cm, (9, 17)), "ld_x < T": put(cm, (1, T - 1)), "ld_m < T": put(cm, (3, T - 1)), "ld_f < T": put(cm, (5, T - 1)),
            "ld_c < T": put(cm, (16, T - 1)),
        },
        "mrx_tod_regress_normal": {
            "null x": put(ne, (0, None)), "null B": put(ne, (10, None)), "null N": put(ne, (13, None)), "null r": put(ne, (14, None)),
            "D 0": put(ne, (6, 0)), "T 0": put(ne, (7, 0)), "G 0": put(ne, (9, 0)), "G 17": put(ne, (9, 17)), "K 0": put(ne, (12, 0)),
            "K 9": put(ne, (12, 9)), "ld_x < T": put(ne, (1, T - 1)), "ld_m < T": put(ne, (3, T - 1)), "ld_f < T": put(ne, (5, T - 1)),
            "ld_b < T": put(ne, (11, T - 1)),
        },
        "mrx_tod_regress_apply": {
            "null x": put(ap, (0, None)), "null B": put(ap, (6, None)), "null a": put(ap, (9, None)), "null y": put(ap, (11, None)),
            "D 0": put(ap, (2, 0)), "T 0": put(ap, (3, 0)), "G 0": put(ap, (5, 0)), "G 17": put(ap, (5, 17)), "K 0": put(ap, (8, 0)),
            "K 9": put(ap, (8, 9)), "sign 0": put(ap, (10, 0)), "sign 2": put(ap, (10, 2)), "ld_x < T": put(ap, (1, T - 1)),
            "ld_y < T": put(ap, (12, T - 1)), "ld_b < T": put(ap, (7, T - 1)), "in place at another pitch": put(ap, (11, ptr(x)), (12, T + 4)),
        },
    }
    for entry, bad in cases.items():
        for name, args in bad.items():
            assert getattr(lib, entry)(hd, *args) == -1, (entry, name)
            assert entry.encode() in lib.mrx_last_error(hd), (entry, name)
    torch.cuda.synchronize()
    for out in (S, W, mean, N, r, y):
        assert bool((out == 7.0).all())
    assert bool((hits == 12345).all()) and bool((x == 1.0).all())
    # a pitch of an array that is not given is not looked at; each output alone is enough; groups, offsets and hits may be null
    assert lib.mrx_tod_column_mean(hd, *put(cm, (2, None), (3, 0), (4, None), (5, 0), (8, None), (12, None), (13, None), (15, None), (16, 0))) == 0
    torch.cuda.synchronize()
    assert bool((W[0] == float(D)).all()) and bool((W[1] == 0.0).all()) and bool((S == 7.0).all()) and bool((mean == 7.0).all())
    assert lib.mrx_tod_regress_normal(hd, *put(ne, (2, None), (3, 0), (4, None), (5, 0), (8, None), (15, None))) == 0
    torch.cuda.synchronize()
    assert bool((N == float(T)).all()) and bool((r == float(T)).all()) and bool((hits == 12345).all())
    assert lib.mrx_tod_column_mean(hd, *cm) == 0 and lib.mrx_tod_regress_normal(hd, *ne) == 0 and lib.mrx_tod_regress_apply(hd, *ap) == 0
    torch.cuda.synchronize()
    assert S[:, 0].tolist() == [0.0, 0.0] and W[:, 0].tolist() == [2.0, 1.0] and mean[:, 5].tolist() == [0.0, 0.0]  # u (1 - off) = 0
    assert hits.tolist() == [T, T, 0, T] and not bool(N[2].any()) and bool((N[0] == float(T)).all())
    assert bool((y[:, :T] == torch.tensor([-2.0, -2.0, 1.0, -2.0], device=DEV)[:, None]).all()) and bool((y[:, T:] == 7.0).all())


def test_solve_on_the_device(gpu_ctx):
    """regress.solve on device tensors against the reference's solve of the same N and r, within 1e3 K n 2^-52 of the
    row's largest coefficient: the summation bound times the cap on the scaled matrices' condition number
    (test_host_regress.py::test_the_test_templates_are_well_conditioned); and the rows that must come back not ok."""
    import torch

    from maria_amd import regress

    worst = 0.0
    for T in (16, 63, 64, 65, 1023, 1025, 4099):
        for K in range(1, 9):
            if T < 4 * K:
                continue
            D = 5
            x, _, flags, _, _, _ = rows(D, T, T + K, exact=False)
            flags[D - 1, :] = 1  # wholly flagged
            B = templates(1, K, T, 7 * T + K)
            N, r, hits, _, _ = ref.normal_equations(x, B, flags=flags)
            a_ref, ok_ref = ref.solve(N, r, hits, min_hits=1)
            a, ok = regress.solve(*(torch.as_tensor(v).to(DEV) for v in (N, r, hits)), min_hits=1)
            assert a.dtype == torch.float64 and ok.dtype == torch.bool and a.is_cuda
            a, ok = a.cpu().numpy(), ok.cpu().numpy()
            assert ok.tolist() == ok_ref.tolist() == [True] * (D - 1) + [False] and not a[D - 1].any()
            err = np.abs(a - a_ref).max(axis=1) / np.maximum(np.abs(a_ref).max(axis=1), 1e-300)
            tol = 1e3 * K * hits * EPS
            assert np.all(err[:-1] <= tol[:-1]), (T, K, err, tol)
            worst = max(worst, float((err[:-1] / tol[:-1]).max()))
    print(f"max |a - ref| / (1e3 K n 2^-52 max|a|) = {worst:.3g}")
    # fewer samples than templates; a duplicated template; min_hits
    for T, K, dup in ((3, 5, False), (257, 4, True)):
        x, _, _, _, _, _ = rows(3, T, 11, exact=False)
        B = templates(1, K, T, 12)
        if dup:
            B[0, 3] = B[0, 1]
        N, r, hits = regress.normal_equations(torch.as_tensor(x).to(DEV), torch.as_tensor(B).to(DEV), ctx=gpu_ctx)
        a, ok = regress.solve(N, r, hits, min_hits=1)
        assert not bool(ok.any()) and not bool(a.any())
    a, ok = regress.solve(N, r, hits, min_hits=258)
    assert not bool(ok.any())


def injected(D, T, G, seed, drifts):
    """(x, sky, groups, gains, c, extra): x = sky + float32(o_d + g_d c_t (+ Legendre drifts)) put in with apply(sign=+1)."""
    import torch

    from maria_amd import regress

    rng = np.random.default_rng(seed)
    sky = (0.05 * rng.standard_normal((D, T))).astype(np.float32)
    c = np.cumsum(rng.standard_normal((G, T)), axis=1)
    c = (c / np.abs(c).max(axis=1, keepdims=True) * 4).astype(np.float32)
    groups = rng.integers(0, G, D).astype(np.int32)
    groups[1] = -1
    gains = rng.uniform(0.7, 1.3, D)
    for g in range(G):
        gains[groups == g] /= gains[groups == g].mean()  # unit mean within the group: what the fit normalises to
    extra = regress.legendre_templates(T, 2)[1:] if drifts else None
    a = np.column_stack([rng.uniform(-3, 3, D), gains] + ([rng.uniform(-1, 1, (D, 2))] if drifts else []))
    B = np.ones((G, a.shape[1], T), np.float32)
    B[:, 1] = c
    if drifts:
        B[:, 2:] = extra[None]
    x = regress.apply(torch.as_tensor(sky).to(DEV), torch.as_tensor(B).to(DEV), torch.as_tensor(a).to(DEV), groups=groups, sign=+1)
    return x, torch.as_tensor(sky).to(DEV), groups, gains, c, extra


@pytest.mark.parametrize("drifts", [False, True])
def test_an_injected_common_mode_is_taken_out_exactly(gpu_ctx, drifts):
    """x = sky + g_d c_t + o_d (+ drifts), model = sky: fit_common_mode and apply return sky within 8 * 2^-24 max|x| of
    the row (the injection, c's float32 rounding, the rounded combination and the subtraction: a rounding each, and a
    factor 2 to spare); the normalised gains come back within the same bound over the rms of c's part orthogonal to the
    other templates (a least-squares gain is a mean of sample errors weighted by c's orthogonal part: Cauchy-Schwarz).
    Samples flagged in every row and filled with 1e6 change nothing of this."""
    import torch

    from maria_amd import regress

    D, T, G = 63, 1025, 2
    x, sky, groups, gains, c, extra = injected(D, T, G, 3, drifts)
    top = x.abs().max(dim=1).values.cpu().numpy()
    flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    flags[:, 100:140] = 1
    spoiled = x.clone()
    spoiled[:, 100:140] = 1e6
    grouped = groups >= 0
    others = np.vstack([np.ones(T)] + ([extra.astype(np.float64)] if drifts else []))
    for xx, ff in ((x, None), (spoiled, flags)):
        cm, a, g, ok, B = regress.fit_common_mode(xx, groups=groups, n_groups=G, flags=ff, model=sky, extra=extra, min_hits=8, ctx=gpu_ctx)
        y = regress.apply(x, B, a, groups=groups, ctx=gpu_ctx)
        assert ok.cpu().numpy().tolist() == grouped.tolist()
        keep = np.ones(T, bool) if ff is None else ~((np.arange(T) >= 100) & (np.arange(T) < 140))  # the samples that were fitted
        err = (y - sky).abs()[:, torch.as_tensor(keep).to(DEV)].max(dim=1).values.cpu().numpy() / (2.0**-24 * top)
        assert torch.equal(y[1], x[1])  # the row of group -1
        g = g.cpu().numpy()
        rel = np.zeros(D)
        for k in range(G):
            ck = c[k].astype(np.float64)[keep]
            perp = ck - others[:, keep].T @ np.linalg.lstsq(others[:, keep].T, ck, rcond=None)[0]
            rows_k = groups == k
            rel[rows_k] = np.abs(g[rows_k] - gains[rows_k]) / (2.0**-24 * top[rows_k] / np.sqrt(np.mean(perp**2)))
        print(f"drifts {drifts}, flags {ff is not None}: max |y - sky| / (2^-24 max|x|) = {err[grouped].max():.3f}; "
              f"max |gain - injected| / (2^-24 max|x| / rms c_perp) = {rel.max():.3f}")
        assert np.all(err[grouped] <= 8.0) and np.all(rel <= 8.0)


def test_flagged_samples_do_not_touch_the_coefficients(gpu_ctx):
    """Random flags: what the flagged samples hold (the data, 1e6, NaN) changes no bit of c, a, the gains or ok."""
    import torch

    from maria_amd import regress

    D, T, G = 65, 4099, 2
    x, sky, groups, _, _, extra = injected(D, T, G, 4, True)
    flags = torch.as_tensor((np.random.default_rng(5).random((D, T)) < 0.03).astype(np.uint8)).to(DEV)
    flags[7, :] = 1
    results = []
    for fill in (None, 1e6, float("nan")):
        xx = x.clone()
        if fill is not None:
            xx[flags != 0] = fill
        results.append(regress.fit_common_mode(xx, groups=groups, n_groups=G, flags=flags, model=sky, extra=extra, ctx=gpu_ctx))
    ok = results[0][3].cpu().numpy()
    assert not ok[7] and not ok[1] and ok.sum() == D - 2
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


def simulated(duration=60.0, with_map=False):
    """Simulation(atmosphere="2d") of 32 positions x 2 bands on a daisy at 50 Hz, K_RJ; with a compact source as a second
    field for the map test (test_gpu_ground.py's map, behind a 30 m dish)."""
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation, sky_transform_stack

    bands = [Band(center=93e9, width=27e9, shape="top_hat", name="f093"), Band(center=150e9, width=41e9, shape="top_hat", name="f150")]
    n, width = 128, 1.0  # degrees
    inst = Instrument(Detectors.hexagon(32, width / 2, bands, primary_size=30.0))
    site = Site(altitude=5000.0)
    plan = Plan.daisy(start_time=1.7e9, duration=duration, sample_rate=50.0, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
    kw = dict(atmosphere="2d", atmosphere_kwargs={"n_layers": 2, "seed": 4, "pwv_rms_frac": 0.1}, noise=False)
    if not with_map:
        (tod,) = Simulation(inst, plan, site, **kw).run()
        return tod
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    data = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0
    data = (data - data.mean()).astype(np.float32)
    centre = _centre(plan.phi.astype(np.float32), plan.theta.astype(np.float32), sky_transform_stack(plan.time, site.latitude, site.longitude))
    sky = mmap.ProjectionMap(data, nu=150e9, width=width, center=np.degrees(centre), frame="ra/dec")
    (tod,) = Simulation(inst, plan, site, map=sky, **kw).run()
    return tod, sky, centre, bands, n, width / (n - 1)


@pytest.fixture(scope="module")
def atmosphere_tod(gpu_ctx):
    import torch

    tod = simulated()
    assert tod.units == "K_RJ" and tod.fields == ["atmosphere"]
    tod.data = {"atmosphere": torch.as_tensor(tod.data["atmosphere"]).to(DEV, torch.float32)}
    assert tuple(tod.data["atmosphere"].shape) == (64, 3000) and sorted(set(tod.dets.band_index.tolist())) == [0, 1]
    return tod


def host(v):
    import torch

    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def ulps_of_the_combination(got, want, x):
    """max over samples of |got - want| in float32 ulps of the row's largest subtracted value (x - want)."""
    comb = np.abs(x.astype(np.float64) - want.astype(np.float64)).max(axis=1)
    ulp = np.spacing(np.maximum(comb, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp[:, None]).max())


COMMON_MODE_CASES = {
    "band": dict(), "one group": dict(groups=None), "poly": dict(poly_order=2), "airmass": dict(airmass=True, poly_order=1),
    "model": dict(model=True), "into": dict(into="extra"), "left out": dict(groups="some"), "one iteration": dict(n_iter=1),
}


@pytest.mark.parametrize("case", list(COMMON_MODE_CASES))
@pytest.mark.parametrize("chain", ["plain", "flagged and downsampled"])
def test_tod_remove_common_mode_against_the_reference(gpu_ctx, atmosphere_tod, case, chain):
    """TOD.remove_common_mode on a simulated atmosphere against regress_ref.fit_common_mode and apply on the same float32
    signal on the host: within K_ULPS float32 ulps of the subtracted combination; each band's row rms falls."""
    import torch

    from maria_amd import regress
    from maria_amd.sim import TOD

    src = atmosphere_tod
    kw = dict(COMMON_MODE_CASES[case])
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
    kept = {k: host(v).copy() for k, v in tod.data.items()}
    out = tod.remove_common_mode(ctx=gpu_ctx, **kw)
    # the source is as it was; what is carried
    assert "common_mode" not in tod.metadata and all(np.array_equal(host(tod.data[k]), v) for k, v in kept.items())
    assert out.fields == tod.fields and out.flags is tod.flags and out.dets is tod.dets and out.coords is tod.coords and out.units == tod.units
    assert out._calibrator is getattr(tod, "_calibrator", None)
    for v in out.data.values():
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (D, T)
    # the reference on the host, from the same float32 signal
    signal = sum(kept.values()).astype(np.float32) if len(kept) > 1 else kept["atmosphere"]
    groups = band if case not in ("one group", "left out") else (None if case == "one group" else kw["groups"])
    G = 1 if groups is None else 2
    order = kw.get("poly_order", 0)
    extra = [regress.legendre_templates(T, order)[1:]] + ([regress.airmass_template(tod.coords._bel)[None]] if kw.get("airmass") else [])
    extra = np.concatenate(extra)
    flags = None if tod.flags is None else host(tod.flags)
    model = None if kw.get("model") is None else kept["extra"]
    c, a, g, ok, B = ref.fit_common_mode(signal, groups=groups, n_groups=G, flags=flags, model=model, extra=extra if len(extra) else None,
                                         n_iter=kw.get("n_iter", 3), min_hits=8)
    into = kw.get("into", "atmosphere")
    want = ref.apply(kept[into], B, a, groups=groups, sign=-1)
    got = host(out.data[into])
    for name in kept:
        if name != into:
            assert np.array_equal(host(out.data[name]), kept[name]), name
    grouped = np.ones(D, bool) if groups is None else groups >= 0
    assert ok.tolist() == grouped.tolist() and np.array_equal(got[~grouped], kept[into][~grouped])
    meta = out.metadata["common_mode"]
    assert meta["n_groups"] == G and meta["n_iter"] == kw.get("n_iter", 3) and meta["poly_order"] == order and meta["airmass"] == bool(kw.get("airmass"))
    assert meta["common_mode"].dtype == np.float32 and meta["common_mode"].shape == (G, T) and meta["coefficients"].shape == (D, 2 + len(extra))
    assert meta["failed_rows"].size == 0 and np.array_equal(meta["offsets"], meta["coefficients"][:, 0]) and meta["gains"].shape == (D,)
    k = ulps_of_the_combination(got, want, kept[into])
    gain_err = float(np.abs(meta["gains"] - g)[grouped].max())
    before = np.sqrt(((signal - signal.mean(axis=1, keepdims=True)) ** 2).mean(axis=1))
    after_signal = sum(host(v) for v in out.data.values())
    after = np.sqrt(((after_signal - after_signal.mean(axis=1, keepdims=True)) ** 2).mean(axis=1))
    ratios = [float((after[grouped & (band == b)] / before[grouped & (band == b)]).max()) for b in (0, 1)]
    whole = 0.0 if flags is None else float(np.mean([(flags[grouped & (band == b)] != 0).all(axis=0).mean() for b in (0, 1)]))
    print(f"{case}, {chain}: {k:.3f} float32 ulps of the subtracted combination; max |gain - ref| {gain_err:.2e}; "
          f"largest row rms after / before per band {ratios[0]:.3e} {ratios[1]:.3e}; samples flagged in a whole band {whole:.2%}")
    assert k <= K_ULPS
    # the two fits differ by the order of a few float64 sums and by the solver: parts in 1e12 of a gain of order one, far from 1e-6
    assert gain_err <= 1e-6
    assert np.all(after[grouped] < before[grouped])


@pytest.mark.parametrize("chain", ["plain", "flagged and downsampled"])
def test_tod_regress_against_the_reference(gpu_ctx, atmosphere_tod, chain):
    import torch

    from maria_amd import regress
    from maria_amd.sim import TOD

    src = atmosphere_tod
    rng = np.random.default_rng(4)
    data = {"atmosphere": src.data["atmosphere"].clone(), "extra": (0.01 * rng.standard_normal((64, 3000))).astype(np.float32)}
    tod = TOD(data, src.dets, src.coords, units=src.units, metadata=dict(src.metadata))
    if chain != "plain":
        tod = tod.flag_glitches(n_sigma=3.0, ctx=gpu_ctx).downsample(4, ctx=gpu_ctx)
    D, T = tod.data["atmosphere"].shape
    kept = {k: host(v).copy() for k, v in tod.data.items()}
    signal = (kept["atmosphere"] + kept["extra"]).astype(np.float32)
    flags = None if tod.flags is None else host(tod.flags)
    P = regress.legendre_templates(T, 2)
    for kw in (dict(), dict(into="extra"), dict(model=kept["extra"])):
        out = tod.regress(P, ctx=gpu_ctx, **kw)
        assert "regress" not in tod.metadata and all(np.array_equal(host(tod.data[k]), v) for k, v in kept.items())
        assert out.flags is tod.flags and out.dets is tod.dets and out.coords is tod.coords and out.units == tod.units
        for v in out.data.values():
            assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (D, T)
        N, r, hits, _, _ = ref.normal_equations(signal, P[None], flags=flags, model=kw.get("model"))
        a, ok = ref.solve(N, r, hits, min_hits=8)
        into = kw.get("into", "atmosphere")
        want = ref.apply(kept[into], P[None], a, sign=-1)
        other = "extra" if into == "atmosphere" else "atmosphere"
        assert ok.all() and np.array_equal(host(out.data[other]), kept[other])
        meta = out.metadata["regress"]
        assert meta["n_templates"] == 3 and meta["failed_rows"].size == 0 and meta["coefficients"].shape == (D, 3)
        assert np.abs(meta["coefficients"] - a).max() <= 1e3 * 3 * T * EPS * np.abs(a).max()
        k = ulps_of_the_combination(host(out.data[into]), want, kept[into])
        print(f"regress {sorted(kw)}, {chain}: {k:.3f} float32 ulps of the subtracted combination")
        assert k <= K_ULPS
    # too few samples for a row: it is left as it is, and named
    few = torch.zeros((D, T), dtype=torch.uint8, device=DEV) if tod.flags is None else tod.flags.clone()
    few[5, 6:] = 1
    tod.flags = few
    out = tod.regress(P, ctx=gpu_ctx)
    assert out.metadata["regress"]["failed_rows"].tolist() == [5] and np.array_equal(host(out.data["atmosphere"])[5], kept["atmosphere"][5])


def test_a_second_removal_changes_nothing(gpu_ctx):
    """The removal is a projection: remove_common_mode of its own result, with the same model, moves no sample by more
    than 8 * 2^-24 max|x| of the row (the bound of test_an_injected_common_mode_is_taken_out_exactly)."""
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    D, T, G = 63, 1025, 2
    x, sky, groups, _, _, _ = injected(D, T, G, 6, True)
    t = 1.7e9 + np.arange(T) / 50.0
    dets = Detectors(np.zeros((D, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int))
    tod = TOD({"signal": x}, dets, Coordinates(t, np.zeros(T), np.full(T, 1.0)), units="K_RJ")
    once = tod.remove_common_mode(groups=groups, poly_order=2, model=sky, ctx=gpu_ctx)
    twice = once.remove_common_mode(groups=groups, poly_order=2, model=sky, ctx=gpu_ctx)
    top = x.abs().max(dim=1).values
    first = float(((once.data["signal"] - sky).abs().max(dim=1).values / (2.0**-24 * top)).max())
    moved = float(((twice.data["signal"] - once.data["signal"]).abs().max(dim=1).values / (2.0**-24 * top)).max())
    print(f"|once - sky| / (2^-24 max|x|) = {first:.3f}; moved by a second removal / (2^-24 max|x|) = {moved:.3f}")
    assert first <= 8.0 and moved <= 8.0
    assert once.metadata["common_mode"]["failed_rows"].size == 0


def test_the_map_through_the_atmosphere(gpu_ctx):
    """A compact source under a simulated atmosphere, binned on the input map's grid from the raw TOD and from
    remove_common_mode(groups="band"): the weighted rms residual per band against the input map falls.  (DESIGN 3.22
    holds both.)"""
    from maria_amd.mappers import BinMapper

    tod, sky, centre, bands, n, res = simulated(with_map=True)
    assert set(tod.fields) == {"atmosphere", "map"} and tod.units == "K_RJ"
    cleaned = tod.remove_common_mode(groups="band", into="atmosphere", ctx=gpu_ctx)
    residual = {}
    for name, t in (("raw", tod), ("cleaned", cleaned)):
        mapper = BinMapper([t], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="I",
                           nu=[b.center for b in bands], frame="ra/dec", units="K_RJ")
        out = mapper.run()
        assert out.data.shape[-2:] == (n, n) and np.allclose(out.xi, sky.xi, atol=1e-12) and np.allclose(out.eta, sky.eta, atol=1e-12)
        m0, m1 = sky.data[0, 0], out.data[0, :]
        w = mapper.products["weight"][0, -1]
        assert (w > 0).mean() > 0.2
        residual[name] = np.sqrt(np.nansum(w * (m1 - m0) ** 2, axis=(-1, -2)) / np.nansum(w))
    print("weighted rms residual per band [K_RJ]: raw", residual["raw"], "after remove_common_mode", residual["cleaned"])
    assert residual["raw"].shape == (2,) and np.all(residual["cleaned"] < residual["raw"])
