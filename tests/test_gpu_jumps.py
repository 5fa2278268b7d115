"""mrx_tod_step_stat, mrx_tod_jump_find, mrx_tod_jump_height, mrx_tod_jump_fix, maria_amd.jumps and TOD.fix_jumps on the
device, against the numpy reference of tests/jumps_ref.py.

The statistic is a float64 value rounded once to float32.  Device and reference form the float64 value in different
orders (prefix sums over a tile, cumulative sums over the row), so the two roundings either agree or differ by one
float32 ulp of s, which is <= 2^-23 |s|.  The statistic's rows are positive (noise about +5, flagged samples +50 on top),
so both means are positive and |s| <= max(|mean_L|, |mean_R|): the bound 2^-23 max(|mean_L|, |mean_R|) holds for such rows
whatever the order of the sums.  On rows of small integers every sum is exact and the results are equal bit for bit.  The
finder and the fix are comparisons and one rounded subtraction: bit for bit.  The heights stay float64: two sums of <= w
terms of magnitude <= max|x| in different orders differ by <= w 2^-52 max|x| each."""

import functools

import flagging_ref
import jumps_ref as ref
import numpy as np
import pytest
from test_gpu_downsample import _centre, hand_tod
from test_host_jumps import RECOVERY, SEEDS, recovery_conditions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 1  # of the jumps of test_the_map_through_jumps
LAYOUTS = ("aligned", "odd")  # rows that allow 16-byte (flags: 4-byte) accesses, and rows that do not


def S():
    from maria_amd import jumps

    return jumps.TILE_SAMPLES


def lengths(w):
    s = S()
    return [1, 2, w, 2 * w, 2 * w + 1, s - 1, s, s + 1, 2 * s + w + 3, 3 * s + 17]


def device_rows(a, layout, fill):
    """The [D, T] array ``a`` on the device inside a buffer filled with ``fill``: (buffer, view, pitch).  "aligned": the
    pitch the next multiple of 4 elements, no offset; "odd": a pitch of T + 3 (+ 1 if that is a multiple of 4) and an
    offset of one element, so that neither pointer nor pitch allows a wide access."""
    import torch

    a = np.asarray(a)
    D, T = a.shape
    if layout == "aligned":
        pitch, offset = (T + 3) // 4 * 4, 0
    else:
        pitch, offset = T + 3 + ((T + 3) % 4 == 0), 1
    buf = torch.full((offset + D * pitch + 64,), fill, dtype=torch.as_tensor(a[:0]).dtype, device=DEV)
    view = torch.as_strided(buf, (D, T), (pitch, 1), offset)
    view.copy_(torch.as_tensor(a))
    return buf, view, pitch


def untouched_outside(buf, view, fill):
    """Was nothing but the view written?  (Fills the view; call after reading it.)"""
    view.fill_(fill)
    return bool((buf == fill).all())


def positive_rows(D, T, seed, integers=False):
    """(x, flags): noise about +5 (``integers``: integers of -64 .. 64) with 2 % of the samples flagged at random and
    carrying +50, a flagged run of 300 samples from 40 on in row 0, and (D > 2) row 1 flagged end to end."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-64, 65, (D, T)).astype(np.float32) if integers else (rng.standard_normal((D, T)) + 5).astype(np.float32)
    f = (rng.random((D, T)) < 0.02).astype(np.uint8) * rng.integers(1, 3, (D, T)).astype(np.uint8)
    f[0, 40:340] = 2
    if D > 2:
        f[1] = 1
    x[f != 0] += 50.0
    return x, f


def run_stat(gpu_ctx, x, f, w, g, layout, min_count=None):
    import torch

    from maria_amd import jumps

    xbuf, xv, _ = device_rows(x, layout, -3.0)
    fbuf, fv = None, None
    if f is not None:
        fbuf, fv, _ = device_rows(f, layout, 0)
    before = xbuf.clone(), None if f is None else fbuf.clone()
    sbuf, sv, _ = device_rows(np.full(x.shape, 7.0, np.float32), layout, 7.0)
    out = jumps.step_statistic(xv, w, g, flags=fv, min_count=min_count, ctx=gpu_ctx, out=sv)
    torch.cuda.synchronize()
    assert out is sv and torch.equal(xbuf, before[0]) and (f is None or torch.equal(fbuf, before[1])), "an input changed"
    got = sv.cpu().numpy()
    assert untouched_outside(sbuf, sv, 7.0), "written outside the rows"
    return got


@pytest.mark.parametrize("D", [1, 3, 65])
@pytest.mark.parametrize("w,g", [(2, 0), (32, 4), (256, 64)])
def test_statistic(gpu_ctx, w, g, D):
    worst = 0.0
    for T in lengths(w):
        x, f = positive_rows(D, T, seed=T + D + w)
        xi, fi = positive_rows(D, T, seed=T + D + w + 1, integers=True)
        for flags, flags_i in ((None, None), (f, fi)):
            want, scale = ref.step_statistic(x, w, g, flags)
            want_i, _ = ref.step_statistic(xi, w, g, flags_i)
            if flags is None and T >= 2 * w + 1:
                assert want.any(), (T, "the reference forms no statistic")
            if flags is not None and D > 2:
                assert not want[1].any()  # a row flagged end to end
            if flags is not None and T > 400 and w <= 32:
                assert not want[0, 100:280].any() and not scale[0, 100:280].any()  # too few valid samples on a side
            for layout in LAYOUTS:
                got = run_stat(gpu_ctx, x, flags, w, g, layout)
                formed = scale > 0
                assert not got[~formed].any(), (T, layout, "not exactly 0 where a side has fewer than min_count samples")
                err = np.abs(got.astype(np.float64) - want)[formed] / (2.0**-23 * scale[formed])
                if err.size:
                    worst = max(worst, float(err.max()))
                    assert err.max() <= 1.0, (T, layout, float(err.max()))
                got_i = run_stat(gpu_ctx, xi, flags_i, w, g, layout)
                assert np.array_equal(got_i, want_i), (T, layout, int((got_i != want_i).sum()))
    print(f"w {w} g {g} D {D}: max |gpu - ref| / (2^-23 max(|mean_L|, |mean_R|)) = {worst:.3f}")


def test_statistic_min_count_and_no_out(gpu_ctx):
    """min_count 1 and window: the count test is >=; out=None allocates; rows shorter than the window give zeros."""
    import torch

    from maria_amd import jumps

    x, f = positive_rows(3, S() + 9, seed=2, integers=True)
    for m in (1, 16):
        want, _ = ref.step_statistic(x, 16, 2, f, m)
        got = jumps.step_statistic(torch.as_tensor(x).to(DEV), 16, 2, flags=torch.as_tensor(f).to(DEV), min_count=m, ctx=gpu_ctx)
        assert np.array_equal(got.cpu().numpy(), want), m
    short = torch.ones((2, 7), dtype=torch.float32, device=DEV)
    assert not jumps.step_statistic(short, 16, ctx=gpu_ctx).any()


HAND = (0, 1, -2, -1)  # hand-placed peaks at the row ends; and at S - 1, S, S + 4, S + 64 and S + sep


def find_case(D, T, sep, seed):
    """(s, thresh): a quantised statistic (ties and plateaus in every window) with large values placed by hand at
    0, 1, T - 2, T - 1, S - 1, S, S + sep and S + grow_after for every grow_after of the test (0, 4, 64) in row 0 and, negated,
    in the last row; row 1 (D > 2) zeros with threshold 0, row 2 (D > 3) a NaN threshold; the other thresholds 2.5."""
    s0 = S()
    s = ref.quantised_statistic(D, T, seed)
    for k, t in enumerate([T + h if h < 0 else h for h in HAND] + [s0 - 1, s0, s0 + 4, s0 + 64, s0 + sep]):
        if 0 <= t < T:
            s[0, t] = 40.0 + k % 3
            s[-1, t] = -(40.0 + (k + 1) % 3)
    thresh = np.full(D, 2.5, np.float32)
    if D > 2:
        s[1], thresh[1] = 0.0, 0.0
    if D > 3:
        thresh[2] = np.nan
    return s, thresh


@functools.lru_cache(maxsize=None)
def find_reference(D, T, sep):
    s, thresh = find_case(D, T, sep, seed=T + D + sep)
    peaks, n = ref.find(s, thresh, sep, 0, 0)
    return s, thresh, peaks, n


def grown(peaks, before, after):
    """The reference's flags for a grow, from its peaks (ref.find with no grow): the same loops."""
    D, T = peaks.shape
    out = np.zeros((D, T), np.uint8)
    for d, p in zip(*np.nonzero(peaks)):
        out[d, max(0, p - before):min(T, p + after + 1)] = 2
    out[peaks != 0] = 1
    return out


def run_find(gpu_ctx, s, thresh, sep, grow, layout, count=True):
    import torch

    from maria_amd._lib import ptr

    D, T = s.shape
    sbuf, sv, ld_s = device_rows(s, layout, -3.0)
    before = sbuf.clone()
    fbuf, fv, ld_f = device_rows(np.full((D, T), 9, np.uint8), layout, 9)
    d_thresh = torch.as_tensor(np.asarray(thresh, np.float32)).to(DEV)
    d_count = torch.full((D,), 12345, dtype=torch.int32, device=DEV)  # overwritten, not accumulated
    gpu_ctx.call("mrx_tod_jump_find", ptr(sv), ld_s, D, T, ptr(d_thresh), sep, grow[0], grow[1], ptr(fv), ld_f, ptr(d_count) if count else None)
    torch.cuda.synchronize()
    assert torch.equal(sbuf, before), "the input changed"
    got = fv.cpu().numpy()
    assert untouched_outside(fbuf, fv, 9), "written outside the rows"
    return got, d_count.cpu().numpy()


@pytest.mark.parametrize("sep", [1, 32, 512])
def test_finder_bit_for_bit(gpu_ctx, sep):
    assert ref.find(np.full((1, 20), 2.5, np.float32), [0.0], 4, 0, 0)[1][0] == 1  # constants other than 0: the first sample
    for T in lengths(32):
        for D in (1, 3, 65):
            s, thresh, peaks, n_want = find_reference(D, T, sep)
            if T > S() + 64:
                assert n_want[0] >= 3 and n_want[-1] >= 3
            if D > 2:
                assert n_want[1] == 0
            if D > 3:
                assert n_want[2] == 0
            for grow in ((0, 0), (4, 4), (64, 64), (0, 64)):
                want = grown(peaks, *grow)
                if grow == (4, 4) and T <= S():
                    np.testing.assert_array_equal(want, ref.find(s, thresh, sep, 4, 4)[0])
                for layout in LAYOUTS:
                    got, n_got = run_find(gpu_ctx, s, thresh, sep, grow, layout)
                    assert np.array_equal(got, want), (T, D, grow, layout, int((got != want).sum()))
                    assert np.array_equal(n_got, n_want), (T, D, grow, layout)


def test_finder_without_a_count_and_with_a_nan_threshold(gpu_ctx):
    T = 2 * S() + 9
    s = ref.quantised_statistic(2, T, 4)
    want, n_want = ref.find(s, [np.nan, 0.0], 8, 3, 3)
    assert n_want[0] == 0 and n_want[1] > 10
    got, n = run_find(gpu_ctx, s, [np.nan, 0.0], 8, (3, 3), "odd", count=False)
    assert np.array_equal(got, want) and (n == 12345).all()
    got, n = run_find(gpu_ctx, s, [np.nan, 0.0], 8, (3, 3), "aligned")
    assert np.array_equal(got, want) and np.array_equal(n, n_want)
    got, n = run_find(gpu_ctx, np.zeros((1, T), np.float32), [0.0], 8, (3, 3), "aligned")  # a row of constants, threshold 0
    assert not got.any() and n[0] == 0


def height_case(w, g, seed, integers=False):
    """(x, flags, row_start, pos) of 6 rows of T = 2 S + w + 3: row 0 jumps at 0, T - 1 and well apart in between; row 1
    neighbours closer than w + 2 g (clipped windows) and closer than 2 g (empty ones); row 2 none; row 3 one jump whose
    window before it is flagged but for a sample (``ok`` false) and one whose windows are flagged in part; row 4 jumps either
    side of the tile seams; row 5 one jump, no flags near it."""
    s = S()
    T = 2 * s + w + 3
    x, f = positive_rows(6, T, seed, integers)
    x[f != 0] -= 50.0
    f[:] = (np.random.default_rng(seed + 1).random((6, T)) < 0.02)
    rows = [
        [0, 3 * w + 2 * g, s + 5, T - 1],
        [500, 500 + w // 2 + 2 * g, 500 + w + 2 * g + 3, 1500, 1500 + max(1, g), 1900, 1900 + w + 2 * g - 1],
        [],
        [700, 1700],
        [s - 1, s, 2 * s - 1, 2 * s],
        [1234],
    ]
    f[3, 700 - g - w:700 - g - 1] = 1
    f[3, 1700 - g - w // 4:1700 - g] = 2
    f[3, 1700 + g:1700 + g + w // 3] = 2
    f[5, 1234 - g - w:1234 + g + w] = 0
    x[f != 0] += 50.0
    for d, ps in enumerate(rows):
        for k, p in enumerate(ps):
            x[d, p:] += (-1) ** k * (8 + k)
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return x, f, row_start, np.asarray([p for r in rows for p in r], np.int32)


@pytest.mark.parametrize("w,g", [(2, 0), (32, 4), (256, 64)])
def test_heights(gpu_ctx, w, g):
    import torch

    from maria_amd import jumps

    for integers in (False, True):
        x, f, row_start, pos = height_case(w, g, seed=w + g, integers=integers)
        for flags in (None, f):
            want, ok_want = ref.heights(x, row_start, pos, w, g, flags)
            if flags is not None and w >= 32:
                j = row_start[3]
                assert not ok_want[j] and want[j] == 0.0 and ok_want[j + 1] and ok_want[row_start[5]]
            assert ok_want.sum() >= 3
            for layout in LAYOUTS:
                xbuf, xv, _ = device_rows(x, layout, -3.0)
                fv = None if flags is None else device_rows(flags, layout, 0)[1]
                before = xbuf.clone()
                got, ok = jumps.jump_heights(xv, row_start, pos, w, g, flags=fv, ctx=gpu_ctx)
                again, _ = jumps.jump_heights(xv, torch.as_tensor(row_start), torch.as_tensor(pos).to(DEV), w, g, flags=fv, ctx=gpu_ctx)
                torch.cuda.synchronize()
                assert torch.equal(xbuf, before) and got.dtype == torch.float64 and ok.dtype == torch.bool
                assert torch.equal(got, again), "two calls differ"
                got, ok = got.cpu().numpy(), ok.cpu().numpy()
                np.testing.assert_array_equal(ok, ok_want)
                assert not got[~ok].any()
                if integers:
                    np.testing.assert_array_equal(got, want)
                else:
                    bound = 2 * w * 2.0**-52 * float(np.abs(x).max())
                    assert np.abs(got - want).max() <= bound, (layout, float(np.abs(got - want).max()), bound)
    # n = 0: a valid call that does nothing
    h, ok = jumps.jump_heights(torch.as_tensor(x).to(DEV), np.zeros(7, np.int32), np.zeros(0, np.int32), w, g, ctx=gpu_ctx)
    assert tuple(h.shape) == (0,) and tuple(ok.shape) == (0,)


def fix_case(seed=0):
    """(x, row_start, pos, height) of 5 rows of T = 3 S + 17: row 0 jumps at 0, either side of every tile seam and at
    T - 1; rows 1 and 4 none; row 2 a hundred; row 3 one at 0 and two on one sample."""
    s = S()
    T = 3 * s + 17
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((5, T)) * 3 + np.linspace(-20.0, 20.0, T)).astype(np.float32)
    rows = [[0, s - 1, s, 2 * s - 1, 2 * s, 3 * s - 1, 3 * s, T - 1], [], sorted(rng.choice(T, 100, replace=False).tolist()), [0, 77, 77], []]
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    pos = np.asarray([p for r in rows for p in r], np.int32)
    return x, row_start, pos, rng.uniform(-16.0, 16.0, pos.size)


def test_fix_bit_for_bit(gpu_ctx):
    import torch

    from maria_amd import jumps

    x, row_start, pos, height = fix_case()
    want = ref.fix(x, row_start, pos, ref.cumulative(row_start, height))
    assert np.array_equal(want[1], x[1]) and np.array_equal(want[4], x[4]) and (want[0] != x[0]).mean() > 0.99
    for layout in LAYOUTS:
        for other in LAYOUTS:
            xbuf, xv, _ = device_rows(x, layout, -3.0)
            before = xbuf.clone()
            ybuf, yv, _ = device_rows(np.full(x.shape, 7.0, np.float32), other, 7.0)
            out = jumps.fix_jumps(xv, row_start, pos, height, out=yv, ctx=gpu_ctx)
            torch.cuda.synchronize()
            assert out is yv and torch.equal(xbuf, before), "the input changed"
            got = yv.cpu().numpy()
            assert np.array_equal(got, want), (layout, other, int((got != want).sum()))
            assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"
        out = jumps.fix_jumps(xv, row_start, pos, torch.as_tensor(height), out=xv, ctx=gpu_ctx)  # in place
        torch.cuda.synchronize()
        assert out is xv and np.array_equal(xv.cpu().numpy(), want), layout
        assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"
    xd = torch.as_tensor(x).to(DEV)
    assert np.array_equal(jumps.fix_jumps(xd, row_start, pos, height, ctx=gpu_ctx).cpu().numpy(), want)  # out=None
    none = jumps.fix_jumps(xd, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0), ctx=gpu_ctx)  # n = 0: a copy
    assert torch.equal(none, xd) and none.data_ptr() != xd.data_ptr()


@pytest.mark.parametrize("seed", SEEDS)
def test_the_chain_on_noisy_rows(gpu_ctx, seed):
    """The host tier's recovery test on the device: the positions are the reference's, the heights within the bound, the
    fixed rows the reference's fix of the same lists bit for bit, and so the recovery conditions hold here too."""
    import torch

    from maria_amd import jumps

    c = RECOVERY
    x, flags, pos, height = ref.noisy_rows(c["D"], c["T"], c["w"], seed)
    r_start, r_pos, r_height, r_ok, r_scale, r_flags = ref.recover(x, flags, c["w"], c["n_sigma"], c["sep"], c["gap"])
    xd, fd = torch.as_tensor(x).to(DEV), torch.as_tensor(flags).to(DEV)
    row_start, p, jump_flags, count = jumps.find_jumps(xd, c["w"], c["n_sigma"], c["sep"], (4, 4), flags=fd, ctx=gpu_ctx,
                                                       scratch_bytes=4 * c["T"] * 7)  # 7 + 7 + 2 rows
    assert row_start.dtype == torch.int32 and p.dtype == torch.int32 and jump_flags.dtype == torch.uint8 and count.dtype == torch.int64
    np.testing.assert_array_equal(row_start.cpu().numpy(), r_start)
    np.testing.assert_array_equal(p.cpu().numpy(), r_pos)
    np.testing.assert_array_equal(jump_flags.cpu().numpy(), r_flags)
    np.testing.assert_array_equal(count.cpu().numpy(), np.diff(r_start))
    h, ok = jumps.jump_heights(xd, row_start, p, c["w"], c["gap"], flags=fd, ctx=gpu_ctx)
    h_host = h.cpu().numpy()
    np.testing.assert_array_equal(ok.cpu().numpy(), r_ok)
    assert np.abs(h_host - r_height).max() <= 2 * c["w"] * 2.0**-52 * float(np.abs(x).max())
    fixed = jumps.fix_jumps(xd, row_start, p, h, ctx=gpu_ctx)
    np.testing.assert_array_equal(fixed.cpu().numpy(), ref.fix(x, r_start, r_pos, ref.cumulative(r_start, h_host)))
    scale = jumps.robust_scale(jumps.step_statistic(xd, c["w"], 0, flags=fd, ctx=gpu_ctx)).cpu().numpy()
    np.testing.assert_array_equal(scale, r_scale)
    worst = recovery_conditions(pos, height, r_start, p.cpu().numpy(), h_host, ok.cpu().numpy(), scale, c["gap"])
    print(f"seed {seed}: worst position error {worst[0]} samples, worst height error {worst[1]:.2f} robust scales")


def test_c_entry_refusals(gpu_ctx):
    """Each refusal of include/mrx.h returns MRX_ERR_INVALID with a message and leaves the outputs untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T = 4, 3000
    x = torch.ones((D, T), dtype=torch.float32, device=DEV)
    x[:, 1500:] = 9.0
    x0 = x.clone()
    fl = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    s = torch.full((D, T), 7.0, dtype=torch.float32, device=DEV)
    y = torch.full((D, T), 7.0, dtype=torch.float32, device=DEV)
    th = torch.ones(D, dtype=torch.float32, device=DEV)
    f = torch.full((D, T), 9, dtype=torch.uint8, device=DEV)
    n = torch.full((D,), 12345, dtype=torch.int32, device=DEV)
    rs = torch.arange(D + 1, dtype=torch.int32, device=DEV)
    ps = torch.full((D,), 1500, dtype=torch.int32, device=DEV)
    cum = torch.full((D,), 8.0, dtype=torch.float64, device=DEV)
    hgt = torch.full((D,), 77.0, dtype=torch.float64, device=DEV)
    ok = torch.full((D,), 9, dtype=torch.uint8, device=DEV)
    lib, hd = gpu_ctx.lib, gpu_ctx.handle
    stat = (ptr(x), T, ptr(fl), T, D, T, 64, 0, 32, ptr(s), T)
    find = (ptr(x), T, D, T, ptr(th), 64, 4, 4, ptr(f), T, ptr(n))
    height = (ptr(x), T, ptr(fl), T, D, T, ptr(rs), ptr(ps), D, 64, 4, 32, ptr(hgt), ptr(ok))
    fix = (ptr(x), T, D, T, ptr(rs), ptr(ps), ptr(cum), D, ptr(y), T)

    def put(args, i, v):
        return args[:i] + (v,) + args[i + 1:]

    cases = {
        "mrx_tod_step_stat": {
            "null x": put(stat, 0, None), "null s": put(stat, 9, None), "D 0": put(stat, 4, 0), "T 0": put(stat, 5, 0),
            "ld_x < T": put(stat, 1, T - 1), "ld_f < T": put(stat, 3, T - 1), "ld_s < T": put(stat, 10, T - 1),
            "window 1": put(stat, 6, 1), "window 257": put(stat, 6, 257), "gap -1": put(stat, 7, -1), "gap 65": put(stat, 7, 65),
            "min_count 0": put(stat, 8, 0), "min_count 65": put(stat, 8, 65), "s is x": put(stat, 9, ptr(x)),
        },
        "mrx_tod_jump_find": {
            "null s": put(find, 0, None), "null thresh": put(find, 4, None), "null flags": put(find, 8, None), "D 0": put(find, 2, 0),
            "T 0": put(find, 3, 0), "ld_s < T": put(find, 1, T - 1), "ld_f < T": put(find, 9, T - 1), "sep 0": put(find, 5, 0),
            "sep 513": put(find, 5, 513), "grow_before -1": put(find, 6, -1), "grow_before 65": put(find, 6, 65),
            "grow_after -1": put(find, 7, -1), "grow_after 65": put(find, 7, 65),
        },
        "mrx_tod_jump_height": {
            "null x": put(height, 0, None), "null row_start": put(height, 6, None), "null pos": put(height, 7, None),
            "null height": put(height, 12, None), "null ok": put(height, 13, None), "D 0": put(height, 4, 0), "T 0": put(height, 5, 0),
            "n -1": put(height, 8, -1), "ld_x < T": put(height, 1, T - 1), "ld_f < T": put(height, 3, T - 1),
            "window 1": put(height, 9, 1), "window 257": put(height, 9, 257), "gap -1": put(height, 10, -1), "gap 65": put(height, 10, 65),
            "min_count 0": put(height, 11, 0), "min_count 65": put(height, 11, 65),
        },
        "mrx_tod_jump_fix": {
            "null x": put(fix, 0, None), "null y": put(fix, 8, None), "null row_start": put(fix, 4, None), "null pos": put(fix, 5, None),
            "null cum": put(fix, 6, None), "D 0": put(fix, 2, 0), "T 0": put(fix, 3, 0), "n -1": put(fix, 7, -1),
            "ld_x < T": put(fix, 1, T - 1), "ld_y < T": put(fix, 9, T - 1), "in place with another pitch": put(put(fix, 8, ptr(x)), 9, T + 1),
        },
    }
    for entry, bad in cases.items():
        for name, args in bad.items():
            assert getattr(lib, entry)(hd, *args) == -1, (entry, name)
            assert entry.encode() in lib.mrx_last_error(hd), (entry, name)
    torch.cuda.synchronize()
    for t, v in ((s, 7.0), (y, 7.0), (f, 9), (n, 12345), (hgt, 77.0), (ok, 9)):
        assert bool((t == v).all())
    assert torch.equal(x, x0)
    # and the same calls in order: a step of 8 at 1500 in every row
    assert lib.mrx_tod_step_stat(hd, *stat) == 0 and lib.mrx_tod_jump_find(hd, *put(find, 0, ptr(s))) == 0
    assert lib.mrx_tod_jump_height(hd, *height) == 0 and lib.mrx_tod_jump_fix(hd, *fix) == 0
    torch.cuda.synchronize()
    assert float(s[0, 1500]) == 8.0 and n.tolist() == [1] * D and bool((f[:, 1500] == 1).all()) and int((f != 0).sum()) == 9 * D
    assert hgt.tolist() == [8.0] * D and ok.tolist() == [1] * D and bool((y == 1.0).all()) and torch.equal(x, x0)
    # bad lists are clamped, never followed outside the arrays
    bad_rs = torch.tensor([-5, 2, 1, 99, 4], dtype=torch.int32, device=DEV)
    bad_ps = torch.tensor([-7, 10 * T, 5, 3], dtype=torch.int32, device=DEV)
    assert lib.mrx_tod_jump_height(hd, *put(put(height, 6, ptr(bad_rs)), 7, ptr(bad_ps))) == 0
    assert lib.mrx_tod_jump_fix(hd, *put(put(fix, 4, ptr(bad_rs)), 5, ptr(bad_ps))) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, x0)


def test_tod_fix_jumps_to_and_downsample(gpu_ctx):
    import torch

    from maria_amd import jumps

    tod, _, _ = hand_tod()  # 6 x 3001: "map" a numpy field, "noise" a device field
    D, T, w, g = 6, 3001, 64, 4
    pos, height = jumps.inject_jumps(tod.data["noise"], 2, (15.0, 30.0), seed=5, margin=2 * w, spacing=3 * w)
    tod._calibrator = lambda data, to_krj: data
    kept = {k: (v.clone() if isinstance(v, torch.Tensor) else v.copy()) for k, v in tod.data.items()}
    out = tod.fix_jumps(ctx=gpu_ctx)
    # the source is as it was
    assert tod.flags is None and "jumps" not in tod.metadata and isinstance(tod.data["map"], np.ndarray)
    for name, v in kept.items():
        assert torch.equal(tod.data[name], v) if isinstance(v, torch.Tensor) else np.array_equal(tod.data[name], v), name
    # the flags are the reference's on the float32 sum of the fields
    host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in kept.items()}
    signal = host["map"] + host["noise"]
    r_start, r_pos, r_height, r_ok, r_scale, r_flags = ref.recover(signal, None, w, 8.0, w, g)
    assert np.array_equal(np.diff(r_start), [2] * D) and np.abs(r_pos.reshape(D, 2) - pos).max() <= g and r_ok.all()
    assert out.flags.dtype == torch.uint8 and out.flags.is_cuda
    np.testing.assert_array_equal(out.flags.cpu().numpy(), r_flags)
    j = out.metadata["jumps"]
    assert (j["window"], j["n_sigma"], j["gap"], j["sep"], j["grow"], j["min_count"], j["n_fit"], j["fill"], j["into"]) == (
        64, 8.0, 4, 64, (4, 4), 32, 4, True, "map")
    np.testing.assert_array_equal(j["counts"], [2] * D)
    assert len(j["positions"]) == D and len(j["heights"]) == D and j["unfixed"] == 0
    np.testing.assert_array_equal(np.concatenate(j["positions"]), r_pos)
    heights = np.concatenate(j["heights"])
    assert np.abs(heights - r_height).max() <= 2 * w * 2.0**-52 * float(np.abs(signal).max())
    assert np.abs(heights.reshape(D, 2) - height).max() <= 5 * r_scale.max()
    assert j["flagged_fraction"] == (r_flags != 0).sum() / (D * T) and out.metadata["latitude"] == -23.0
    assert out.dets is tod.dets and out.coords is tod.coords and out.units == tod.units and out._calibrator is tod._calibrator
    # only ``into`` is stepped; every field is gap-filled with the same flags
    assert out.fields == ["map", "noise"]
    stepped = {"map": ref.fix(host["map"], r_start, r_pos, ref.cumulative(r_start, heights)), "noise": host["noise"]}
    for name in out.fields:
        v = out.data[name]
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32
        want, _, scale = flagging_ref.gap_fill(stepped[name], r_flags, 4)
        err = np.abs(v.cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= 2.0**-23 * scale), name
    raw = tod.fix_jumps(fill=False, into="noise", ctx=gpu_ctx)
    assert torch.equal(raw.flags, out.flags) and np.array_equal(raw.data["map"].cpu().numpy(), host["map"])
    np.testing.assert_array_equal(raw.data["noise"].cpu().numpy(), ref.fix(host["noise"], r_start, r_pos, ref.cumulative(r_start, heights)))
    assert raw.data["noise"] is not tod.data["noise"] and raw.metadata["jumps"]["into"] == "noise"
    # the TOD's own map field as the model: the statistic is that of the noise field alone, the same jumps
    modelled = tod.fix_jumps(model=tod.data["map"], ctx=gpu_ctx)
    np.testing.assert_array_equal(modelled.metadata["jumps"]["counts"], [2] * D)
    assert np.abs(np.concatenate(modelled.metadata["jumps"]["positions"]).reshape(D, 2) - pos).max() <= g
    assert modelled.flags is not None and int((modelled.flags == 1).sum()) == 2 * D
    # flags the TOD already has are kept, and kept out of the means
    tod.flags = torch.zeros((D, T), dtype=torch.uint8, device=DEV)
    tod.flags[2, 7:9] = 1
    tod.flags[3, int(pos[3, 0]) - 20:int(pos[3, 0]) - 10] = 2
    f0 = tod.flags.cpu().numpy()
    both = tod.fix_jumps(ctx=gpu_ctx)
    b_start, b_pos, b_height, b_ok, _, b_flags = ref.recover(signal, f0, w, 8.0, w, g)
    np.testing.assert_array_equal(both.flags.cpu().numpy() != 0, (b_flags != 0) | (f0 != 0))
    np.testing.assert_array_equal(np.concatenate(both.metadata["jumps"]["positions"]), b_pos)
    assert both.metadata["jumps"]["flagged_fraction"] == ((b_flags != 0) | (f0 != 0)).sum() / (D * T)
    # to() and downsample() carry them
    assert out.to("pW").flags is out.flags
    low = out.downsample(4, ctx=gpu_ctx)
    assert low.flags.dtype == torch.uint8 and tuple(low.flags.shape) == (D, 751)
    np.testing.assert_array_equal(low.flags.cpu().numpy(), flagging_ref.downsample_flags(r_flags, 4))


# res(fixed) / res(clean) per band as measured on an MI355X; the test allows 10 % on top for the order of the
# map's float64 atomics, the one thing that varies from run to run.  Without a model the ratio is far above 1: the sky's
# slope across the window biases every height (DESIGN 3.23 states the finding); with the map field as the model it is 1.005.
MEASURED_RATIO = (2.2731, 2.7006, 2.7226)
MEASURED_RATIO_WITH_MODEL = (1.0046, 1.0053, 1.0039)


def test_the_map_through_jumps(gpu_ctx):
    """test_gpu_flagging.py::test_the_map_through_glitches's set-up (300 positions x 3 bands at 50 Hz, a 60 s daisy, no
    atmosphere, white noise of sigma = 2e-4 K_RJ as a second field) with one jump a row (50 - 500 sigma of either sign, at
    least 2 w from the row's ends) in the noise field, binned on the input map's grid three times: clean, jumpy,
    jumpy.fix_jumps().  With res the weighted rms residual per band against the input map: every jump is found within
    ``gap`` samples, none is left unfixed, at most 2 % of the samples are flagged, res(jumpy) >= 3 res(clean) and
    res(fixed) <= 1.1 x the measured ratio x res(clean).  (DESIGN 3.23 holds the three residuals.)  The measured ratio
    is 2.27 / 2.70 / 2.72, above the 1.25 a repair ought to reach: fix_jumps() without a model takes the heights from a signal
    whose sky part changes by up to 16 sigma across a window.  The same call with ``model=`` the map field is binned as
    well: 1.005 / 1.005 / 1.004."""
    import torch

    from maria_amd import jumps
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
    sigma, w, gap = 2e-4, 64, 4
    noise = torch.as_tensor((sigma * np.random.default_rng(21).standard_normal((D, T))).astype(np.float32)).to(DEV)
    clean.data = {"map": torch.as_tensor(clean.data["map"]).to(DEV), "noise": noise}
    jumpy = TOD({"map": clean.data["map"], "noise": noise.clone()}, clean.dets, clean.coords, units="K_RJ", metadata=dict(clean.metadata))
    pos, height = jumps.inject_jumps(jumpy.data["noise"], 1, (50 * sigma, 500 * sigma), seed=SEED, margin=2 * w)
    assert pos.shape == (D, 1) and pos.min() >= 2 * w and pos.max() < T - 2 * w
    fixed = jumpy.fix_jumps(ctx=gpu_ctx)
    meta = fixed.metadata["jumps"]
    found = sum(int(len(p) > 0 and np.abs(p - pos[d, 0]).min() <= gap) for d, p in enumerate(meta["positions"]))
    residual = {}
    modelled = jumpy.fix_jumps(model=clean.data["map"], ctx=gpu_ctx)
    for name, tod in (("clean", clean), ("jumpy", jumpy), ("fixed", fixed), ("modelled", modelled)):
        mapper = BinMapper([tod], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="I",
                           nu=[b.center for b in bands], frame="ra/dec", units="K_RJ")
        out = mapper.run()
        assert out.data.shape[-2:] == (n, n) and np.allclose(out.xi, sky.xi, atol=1e-12) and np.allclose(out.eta, sky.eta, atol=1e-12)
        m0, m1 = sky.data[0, 0], out.data[0, :]
        wgt = mapper.products["weight"][0, -1]
        assert (wgt > 0).mean() > 0.5
        residual[name] = np.sqrt(np.nansum(wgt * (m1 - m0) ** 2, axis=(-1, -2)) / np.nansum(wgt))
    ratio, ratio_m = residual["fixed"] / residual["clean"], residual["modelled"] / residual["clean"]
    print(f"jumps found {found} of {D}, peaks {int(meta['counts'].sum())}, unfixed {meta['unfixed']}, flagged fraction {meta['flagged_fraction']:.4%}; "
          "weighted rms residual per band [K_RJ]: clean", residual["clean"], "jumpy", residual["jumpy"], "fixed", residual["fixed"], "fixed / clean", ratio,
          "with the map field as the model", residual["modelled"], "/ clean", ratio_m)
    assert found == D
    assert meta["unfixed"] == 0
    assert meta["flagged_fraction"] <= 0.02
    assert residual["clean"].shape == (3,)
    assert np.all(residual["jumpy"] >= 3 * residual["clean"])
    assert np.all(ratio <= 1.1 * np.asarray(MEASURED_RATIO))
    assert modelled.metadata["jumps"]["unfixed"] == 0 and int(modelled.metadata["jumps"]["counts"].sum()) == D
    assert np.all(ratio_m <= 1.1 * np.asarray(MEASURED_RATIO_WITH_MODEL))
