"""The TOD post-processing kernels past the first trip of their resident grids.

Every entry below launches at most R = 8 n_cu workgroups (2048 on a 256-CU MI355X) that stride over the work items with
``for (item = blockIdx.x; item < n_items; item += gridDim.x)``.  The tests of the single areas never go round that loop
three times, and most never twice; production (10 000 x 240 000) goes round it about a thousand times.  Here every shape
follows from the device's CU count: n_items >= 2 R + R / 2 + 1, so that some workgroups make three trips, the rest two, and
the last round is partial, with three items a row (two for the inverse's long rows), so that a workgroup's successive items
lie in different rows at different in-row positions.  Each test asserts that inequality before it launches anything.

Per entry: the work item, n_items of the case here at R = 2048, and the largest n_items any older test reaches (counted in
tests/test_gpu_*.py, the front-end tests of 900 x 3000 included: 2700 tiles of 1024, where the older tests reach them only
through TOD methods and compare maps or front-end results, not the kernel's output sample by sample):

  entry                        work item                        here          older kernel tests    grid
  mrx_tod_median_residual      tile of 1024 samples             1707 x 3      65 x 4                <= R
  mrx_tod_glitch_flag          tile of 1024 samples             1707 x 3      65 x 4                <= R
  mrx_tod_gap_fill             tile of 1024 samples             1707 x 3      5 x 5                 <= R
  mrx_tod_step_stat            tile of 1024 samples             1707 x 3      65 x 4                <= 5 n_cu
  mrx_tod_jump_find            tile of 1024 samples             1707 x 3      65 x 4                <= R
  mrx_tod_jump_fix             tile of 1024 samples             1707 x 3      5 x 4                 <= R
  mrx_tod_decimate             256 outputs                      1707 x 3      130 x 5 = 650         <= R (LDS: fewer)
  mrx_tod_demodulate           128 outputs                      1707 x 3      130 x 10 = 1300       <= R (LDS: 4 n_cu here)
  mrx_tod_hwp_modulate         tile of 1024 samples             1707 x 3      66 x 3                <= R
  mrx_tod_onepole_inverse      (row, chunk of 16 tiles)         5121 x 1, 2561 x 2   33 x 3 = 99    <= R
  mrx_tod_column_mean          (group, tile of 1024 samples)    16 x 321      3 x 5                 <= R
  mrx_tod_regress_apply        tile of 1024 samples             1707 x 3      257 x 5 = 1285        <= R
  mrx_tod_bin_reduce           (row, four bins): a workgroup    1707 x 3      65 x 1024 (strides)   <= R
  mrx_tod_bin_apply            tile of 1024 samples             1707 x 3      65 x 5                <= R
  mrx_tod_segment_normal       (row, segment) a WAVE, 4 a wg    1707 x 12 / 4 33 x 14 / 4           <= R
  mrx_tod_segment_apply        tile of 1024 samples             1707 x 3      33 x 5                <= R
  mrx_tod_segment_moments      (row, segment) a WAVE, 4 a wg    1707 x 12 / 4 33 x 14 / 4           <= R
  mrx_tod_segment_flag         tile of 4096 flags               1707 x 3      33 x 2                <= R

The older counts are verified twice: by the shapes in the older files (65 rows of 3 S + 17 samples are 65 x 4 tiles, and so
on), and by a build in which every one of these loops stops after its first trip: of the 260 older tests of the nine files
249 still pass (the eleven that fail: four map tests at 900 x 3000 -- glitches, jumps, the reduced rate, ground pickup --
hwp's end-to-end sky, the 1300-item demodulation, and five tests of mrx_tod_bin_reduce with 4096 bins), and none of the
tests below does.

(mrx_tod_column_mean takes at most 16 groups, so its items come from the time axis: 321 tiles of 30 rows in 15 groups and
one empty group.  mrx_tod_segment_flag's tile is 4096 flags, so its rows are 2 x 4096 + 517 long.)

What each test asserts:
  1. the result against the float64 reference of the operation, under the acceptance the entry's own test file uses (bit
     for bit where that is, else the bound of the reference module); where the reference is a Python loop per item it runs
     on a subset of rows: every twentieth row, the first and the last, and every row that workgroup 0 and workgroup R - 1
     touch on any trip (item = b + k gridDim, gridDim = min(n_items, R));
  2. the whole output, padding included, against the same entry called on consecutive blocks small enough for one trip
     (at most n_cu workgroups, the regime the older tests establish): equal in every bit, per-row counts included;
  3. inputs of out-of-place calls unchanged, nothing written outside the rows, and a second call the same bits."""

import functools
import warnings

import numpy as np
import pytest
from test_gpu_flagging import device_rows, flag_case, untouched_outside

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ("aligned", "odd")  # pitch the next multiple of the wide access in an aligned buffer; pitch T one element in
TILE = 1024                   # mrx_hwp.hip (modulate), mrx_timeconst.hip, mrx_regress.hip, mrx_ground.hip, mrx_subscan.hip
CHUNK_TILES = 16              # mrx_timeconst.hip: tiles of a work item of the inverse out of place
FLAG_TILE = 4096              # mrx_stats.hip: flags of a work item of mrx_tod_segment_flag
WAVES = 4                     # (row, segment) pairs or bins of a workgroup of the wave-per-item kernels
HALF, GROW, N_FIT = 5, (64, 8), 4
WINDOW, GAP, SEP = 32, 4, 32


def resident(gpu_ctx):
    """(n_cu, R, the least n_items): no entry launches more than R = 8 n_cu workgroups."""
    n_cu = int(gpu_ctx.device_info()["n_cu"])
    R = 8 * n_cu
    return n_cu, R, 2 * R + R // 2 + 1


def rows_for(need, per_row):
    return -(-need // per_row)


def strides(n_items, need):
    print(f"{n_items} work items, at least {need} needed")
    assert n_items >= need, f"{n_items} work items: below {need}, the grid would not make three trips"


def place(a, layout, fill, wide=4):
    """(buffer, view, pitch) of the [D, T] array on the device: "aligned" at a pitch that is a multiple of ``wide``
    elements from the buffer's start, "odd" at pitch T (+ 1 if that is a multiple of 4) one element in."""
    T = a.shape[1]
    pitch, offset = (T + (-T) % wide, 0) if layout == "aligned" else (T + (T % 4 == 0), 1)
    with warnings.catch_warnings():  # the shared cases are read-only arrays; they are only read here
        warnings.simplefilter("ignore", UserWarning)
        buf, view = device_rows(a, pitch, offset, fill)
    return buf, view, pitch


def on_device(a):
    import torch

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def three_ways(launch, fresh, D, step):
    """``launch(lo, hi, outs)`` runs the entry on rows lo .. hi - 1 into the views ``outs``; ``fresh()`` gives new outputs as
    [(buffer, view), ..].  One call on all D rows, the same call again, and calls on consecutive blocks of ``step`` rows (one
    trip each): the three sets of buffers are equal in every bit, padding included.  Returns the first."""
    import torch

    big, again, small = fresh(), fresh(), fresh()
    launch(0, D, [v for _, v in big])
    launch(0, D, [v for _, v in again])
    for lo in range(0, D, step):
        launch(lo, min(D, lo + step), [v for _, v in small])
    torch.cuda.synchronize()
    for k, ((b, _), (a, _), (s, _)) in enumerate(zip(big, again, small)):
        assert torch.equal(b, a), f"output {k}: a second identical call gives other bits"
        assert torch.equal(b, s), f"output {k}: {int((b != s).sum())} elements differ from the one-trip calls"
    return big


def traced_rows(D, n_groups, R, row_of):
    """The rows a loop reference runs on: every twentieth, the first, the last, and every row that workgroups 0 and R - 1
    touch on any trip; ``row_of(w)``: the rows of workgroup item w."""
    grid = min(n_groups, R)
    rows = set(range(0, D, 20)) | {0, D - 1}
    for b in (0, R - 1):
        for w in range(b, n_groups, grid):
            rows |= {r for r in row_of(w) if r < D}
    rows = np.array(sorted(rows))
    assert rows.size >= D / 20 and rows[0] == 0 and rows[-1] == D - 1
    return rows


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


# ---- mrx_glitch.hip ----

T3 = 2 * TILE + 517  # three tiles a row, the last one partial


@functools.lru_cache(maxsize=None)
def glitch_case(D):
    """Tied rows with hand-placed spikes at the row ends and either side of the first seam (test_gpu_flagging.flag_case),
    the thresholds at each row's 99.5th percentile, and the reference's residual, flags and counts."""
    import flagging_ref as ref

    x, thresh = flag_case(D, T3, HALF, GROW, seed=D)
    r, _ = ref.median_residual(x, HALF)
    f, n = ref.flags(x, HALF, thresh, *GROW)
    assert (f == 1).sum() > D and not f[1].any() and f[0, TILE] == 1 and f[-1, TILE - 1] == 1
    for a in (x, thresh, r, f, n):
        a.setflags(write=False)
    return x, thresh, r, f, n


@pytest.mark.parametrize("layout", LAYOUTS)
def test_median_residual(gpu_ctx, layout):
    import torch

    from maria_amd import flagging
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // flagging.TILE_SAMPLES)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    x, _, want, _, _ = glitch_case(D)
    xbuf, xv, ld_x = place(x, layout, -3.0)
    before = xbuf.clone()
    ld_r = []

    def fresh():
        buf, view, ld = place(np.full(x.shape, 7.0, np.float32), layout, 7.0)
        ld_r.append(ld)
        return [(buf, view)]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_median_residual", ptr(xv[lo:hi]), ld_x, hi - lo, T3, HALF, ptr(outs[0][lo:hi]), ld_r[0])

    ((rbuf, rv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before), "the input changed"
    got = rv.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert untouched_outside(rbuf, rv, 7.0), "written outside the rows"


@pytest.mark.parametrize("with_count", [True, False])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_glitch_flag(gpu_ctx, layout, with_count):
    """Without d_count a trip ends without the count's barrier: the one at the loop's top alone keeps a trip's staging off
    the window and the bits the trip before still reads."""
    import torch

    from maria_amd import flagging
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // flagging.TILE_SAMPLES)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    x, thresh, _, want, n_want = glitch_case(D)
    xbuf, xv, ld_x = place(x, layout, -3.0)
    before = xbuf.clone()
    d_thresh = on_device(thresh)
    ld_f = []

    def fresh():
        buf, view, ld = place(np.full(x.shape, 9, np.uint8), layout, 9)  # words, and bytes
        ld_f.append(ld)
        count = torch.full((D,), 12345, dtype=torch.int32, device=DEV)  # overwritten, not accumulated
        return [(buf, view), (count, count)]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_glitch_flag", ptr(xv[lo:hi]), ld_x, hi - lo, T3, HALF, ptr(d_thresh[lo:hi]), GROW[0], GROW[1],
                     ptr(outs[0][lo:hi]), ld_f[0], ptr(outs[1][lo:hi]) if with_count else None)

    (fbuf, fv), (count, _) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before), "the input changed"
    got = fv.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(count.cpu().numpy(), n_want) if with_count else bool((count == 12345).all())
    assert untouched_outside(fbuf, fv, 9), "written outside the rows"


@functools.lru_cache(maxsize=None)
def fill_case(D):
    """(x, flags, the reference's fill, counts and scale).  Rows by d % 5, after test_gpu_flagging.fill_case: 0 runs of 1, 2,
    n_fit and S + 3 samples (across a seam), one at t = 0, one ending at T, two an unflagged sample apart; 1 a run of 2 S
    across two seams; 2 flagged end to end; 3 none; 4 random flags of both values at 2 %."""
    import flagging_ref as ref

    s, T = TILE, T3
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((D, T)) * 3 + np.linspace(-20.0, 20.0, T)).astype(np.float32)
    f = np.zeros((D, T), np.uint8)
    for a, n in ((0, 3), (10, 1), (20, 2), (40, N_FIT), (100, 3), (104, 2), (s - 10, s + 3), (T - 5, 5)):
        f[0::5, a:a + n] = 1 + (a % 2)
    f[1::5, 50:50 + 2 * s] = 2
    f[2::5] = 1
    k = f[4::5].shape[0]
    f[4::5] = (rng.random((k, T)) < 0.02) * rng.integers(1, 3, (k, T))
    want, n_want, scale = ref.gap_fill(x, f, N_FIT)
    assert not n_want[2::5].any() and not n_want[3::5].any() and (n_want[1::5] == 2 * s).all() and n_want[0] == 3 + 1 + 2 + N_FIT + 3 + 2 + s + 3 + 5
    for a in (x, f, want, n_want, scale):
        a.setflags(write=False)
    return x, f, want, n_want, scale


@pytest.mark.parametrize("layout", LAYOUTS)
def test_gap_fill_in_place(gpu_ctx, layout):
    import torch

    from maria_amd import flagging
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // flagging.TILE_SAMPLES)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    x, f, want, n_want, scale = fill_case(D)
    fbuf, fv, ld_f = place(f, layout, 0)  # read as words, and as bytes
    f_before = fbuf.clone()
    ld_x = []

    def fresh():
        buf, view, ld = place(x, layout, -3.0)
        ld_x.append(ld)
        filled = torch.full((D,), 12345, dtype=torch.int32, device=DEV)
        return [(buf, view), (filled, filled)]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_gap_fill", ptr(outs[0][lo:hi]), ld_x[0], hi - lo, T3, ptr(fv[lo:hi]), ld_f, N_FIT, ptr(outs[1][lo:hi]))

    (xbuf, xv), (filled, _) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(fbuf, f_before), "the flags changed"
    got = xv.cpu().numpy()
    keep = (f == 0) | (np.arange(D) % 5 == 2)[:, None]
    assert np.array_equal(got[keep], x[keep]), "an unflagged sample, or a row flagged end to end, changed"
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err[~keep] / (2.0**-23 * scale[~keep])).max())
    print(f"{layout}: max |gpu - ref| / (2^-23 max(|yL|, |yR|)) = {worst:.3f}")
    assert worst <= 1.0
    assert np.array_equal(filled.cpu().numpy(), n_want)
    assert untouched_outside(xbuf, xv, -3.0), "written outside the rows"


# ---- mrx_jumps.hip ----

@functools.lru_cache(maxsize=None)
def stat_case(D, integers):
    import jumps_ref as ref
    from test_gpu_jumps import positive_rows

    x, f = positive_rows(D, T3, seed=D + integers, integers=integers)
    want, scale = ref.step_statistic(x, WINDOW, GAP, f)
    assert want.any() and not want[1].any() and not want[0, 100:280].any()
    for a in (x, f, want, scale):
        a.setflags(write=False)
    return x, f, want, scale


@pytest.mark.parametrize("integers", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_step_statistic(gpu_ctx, layout, integers):
    """Positive Gaussian rows within 2^-23 max(|mean_L|, |mean_R|), rows of small integers bit for bit; flags at 2 %, a
    flagged run, a row flagged end to end."""
    import torch

    from maria_amd import jumps
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // jumps.TILE_SAMPLES)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    x, f, want, scale = stat_case(D, integers)
    xbuf, xv, ld_x = place(x, layout, -3.0)
    fbuf, fv, ld_f = place(f, layout, 0)
    before = xbuf.clone(), fbuf.clone()
    ld_s = []

    def fresh():
        buf, view, ld = place(np.full(x.shape, 7.0, np.float32), layout, 7.0)
        ld_s.append(ld)
        return [(buf, view)]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_step_stat", ptr(xv[lo:hi]), ld_x, ptr(fv[lo:hi]), ld_f, hi - lo, T3, WINDOW, GAP, WINDOW // 2,
                     ptr(outs[0][lo:hi]), ld_s[0])

    ((sbuf, sv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before[0]) and torch.equal(fbuf, before[1]), "an input changed"
    got = sv.cpu().numpy()
    if integers:
        assert np.array_equal(got, want), int((got != want).sum())
    else:
        formed = scale > 0
        assert not got[~formed].any(), "not exactly 0 where a side has fewer than min_count samples"
        err = np.abs(got.astype(np.float64) - want)[formed] / (2.0**-23 * scale[formed])
        print(f"{layout}: max |gpu - ref| / (2^-23 max(|mean_L|, |mean_R|)) = {float(err.max()):.3f}")
        assert err.max() <= 1.0
    assert untouched_outside(sbuf, sv, 7.0), "written outside the rows"


@functools.lru_cache(maxsize=None)
def find_case_here(D):
    """test_gpu_jumps.find_case (hand-placed peaks at the row ends and around the first seam in the first and the last row,
    a row of zeros with threshold 0, a NaN threshold) with the other thresholds at 5.5: about one peak in 65 samples."""
    import jumps_ref as ref
    from test_gpu_jumps import find_case

    s, thresh = find_case(D, T3, SEP, seed=D)
    thresh[thresh == 2.5] = 5.5
    want, n_want = ref.find(s, thresh, SEP, 4, 64)
    assert n_want[0] >= 3 and n_want[-1] >= 3 and n_want[1] == 0 and n_want[2] == 0 and np.median(n_want) >= 5
    for a in (s, thresh, want, n_want):
        a.setflags(write=False)
    return s, thresh, want, n_want


@pytest.mark.parametrize("with_count", [True, False])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_jump_find(gpu_ctx, layout, with_count):
    """Without d_count a trip ends without the count's barrier, as in test_glitch_flag."""
    import torch

    from maria_amd import jumps
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // jumps.TILE_SAMPLES)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    s, thresh, want, n_want = find_case_here(D)
    sbuf, sv, ld_s = place(s, layout, -3.0)
    before = sbuf.clone()
    d_thresh = on_device(thresh)
    ld_f = []

    def fresh():
        buf, view, ld = place(np.full(s.shape, 9, np.uint8), layout, 9)
        ld_f.append(ld)
        count = torch.full((D,), 12345, dtype=torch.int32, device=DEV)
        return [(buf, view), (count, count)]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_jump_find", ptr(sv[lo:hi]), ld_s, hi - lo, T3, ptr(d_thresh[lo:hi]), SEP, 4, 64, ptr(outs[0][lo:hi]), ld_f[0],
                     ptr(outs[1][lo:hi]) if with_count else None)

    (fbuf, fv), (count, _) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(sbuf, before), "the input changed"
    got = fv.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(count.cpu().numpy(), n_want) if with_count else bool((count == 12345).all())
    assert untouched_outside(fbuf, fv, 9), "written outside the rows"


@functools.lru_cache(maxsize=None)
def fix_case_here(D):
    """Rows by d % 4: 0 no jump; 1 one; 2 forty at random; 3 at 0, either side of every seam, two on one sample, and T - 1."""
    import jumps_ref as ref

    s, T = TILE, T3
    rng = np.random.default_rng(D + 1)
    x = (rng.standard_normal((D, T)) * 3 + np.linspace(-20.0, 20.0, T)).astype(np.float32)
    rows = []
    for d in range(D):
        rows.append([[], [int(rng.integers(0, T))], sorted(rng.choice(T, 40, replace=False).tolist()),
                     [0, 77, 77, s - 1, s, 2 * s - 1, 2 * s, T - 1]][d % 4])
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    pos = np.asarray([p for r in rows for p in r], np.int32)
    cum = ref.cumulative(row_start, rng.uniform(-16.0, 16.0, pos.size))
    want = ref.fix(x, row_start, pos, cum)
    assert np.array_equal(want[0::4], x[0::4]) and (want[3::4] != x[3::4]).mean() > 0.99
    for a in (x, row_start, pos, cum, want):
        a.setflags(write=False)
    return x, row_start, pos, cum, want


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_jump_fix(gpu_ctx, layout, in_place):
    import torch

    from maria_amd import jumps
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // jumps.TILE_SAMPLES)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    x, row_start, pos, cum, want = fix_case_here(D)
    xbuf, xv, ld_x = place(x, layout, -3.0)
    before = xbuf.clone()
    d_start, d_pos, d_cum = on_device(row_start), on_device(pos), on_device(cum)
    fill = -3.0 if in_place else 7.0
    ld_y = []

    def fresh():
        buf, view, ld = place(x if in_place else np.full(x.shape, 7.0, np.float32), layout, fill)
        ld_y.append(ld)
        return [(buf, view)]

    def launch(lo, hi, outs):
        src = outs[0] if in_place else xv
        gpu_ctx.call("mrx_tod_jump_fix", ptr(src[lo:hi]), ld_x, hi - lo, T3, ptr(d_start[lo:]), ptr(d_pos), ptr(d_cum), pos.size,
                     ptr(outs[0][lo:hi]), ld_y[0])

    ((ybuf, yv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before), "the input changed"
    got = yv.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert untouched_outside(ybuf, yv, fill), "written outside the rows"


# ---- mrx_decimate.hip, mrx_hwp.hip ----

def by_row_blocks(f, D, step=128):
    """The vectorised reference ``f(lo, hi)`` of rows lo .. hi - 1, block after block (its windows of all rows at once
    would take 700 MB): the tuple of its results, stacked."""
    parts = [f(lo, min(D, lo + step)) for lo in range(0, D, step)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))


@functools.lru_cache(maxsize=None)
def decimate_case(D, T, q, n_taps):
    from test_gpu_downsample import lowpass, noise_rows, reference, tolerance

    x = noise_rows(D, T, seed=D)
    h = lowpass(n_taps, q)
    _, den = reference(x[:1], q, h)
    (want,) = by_row_blocks(lambda lo, hi: (reference(x[lo:hi], q, h)[0],), D)
    tol = tolerance(want, x, h, den)
    for a in (x, h, want, tol):
        a.setflags(write=False)
    return x, h, want, tol


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decimate(gpu_ctx, layout):
    import torch

    from maria_amd import downsample
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    q, n_taps = 4, 81
    T_out = 2 * downsample.TILE_OUTPUTS + 131
    T = q * T_out - 1
    assert downsample.output_length(T, q) == T_out
    per_row = -(-T_out // downsample.TILE_OUTPUTS)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    x, h, want, tol = decimate_case(D, T, q, n_taps)
    xbuf, xv, ld_x = place(x, layout, -3.0)
    before = xbuf.clone()
    d_h = on_device(h)
    ld_y = []

    def fresh():
        buf, view, ld = place(np.full((D, T_out), 7.0, np.float32), layout, 7.0)
        ld_y.append(ld)
        return [(buf, view)]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_decimate", ptr(xv[lo:hi]), ld_x, hi - lo, T, q, ptr(d_h), n_taps, ptr(outs[0][lo:hi]), ld_y[0])

    ((ybuf, yv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before), "the input changed"
    got = yv.cpu().numpy()
    worst = float((np.abs(got.astype(np.float64) - want) / tol).max())
    print(f"{layout}: max |y - ref| / tolerance = {worst:.3f}")
    assert worst <= 1.0
    assert untouched_outside(ybuf, yv, 7.0), "written outside the rows"


@functools.lru_cache(maxsize=None)
def demodulate_case(D, T, q, n_taps):
    import hwp_ref as ref
    from test_gpu_hwp import noise_rows, random_carrier, two_lowpasses

    x, c = noise_rows(D, T, seed=D), random_carrier(T, seed=D + 1)
    ht, hp = two_lowpasses(n_taps, q)
    want = by_row_blocks(lambda lo, hi: ref.demodulate(x[lo:hi], c, q, ht, hp)[:3], D)
    den_t, den_p = ref.denominators(ht, T, q), ref.denominators(hp, T, q)
    peak = np.abs(x).max(axis=0).astype(np.float64)  # max|c x| of a column is |c| max|x|: the product is monotone
    tols = (ref.tolerance_t(want[0], x, ht, den_t), ref.tolerance_p(want[1], np.abs(c[:, 0]) * peak, hp, den_p),
            ref.tolerance_p(want[2], np.abs(c[:, 1]) * peak, hp, den_p))
    for a in (x, c, ht, hp) + want + tols:
        a.setflags(write=False)
    return x, c, ht, hp, want, tols


@pytest.mark.parametrize("want_t", [True, False])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_demodulate(gpu_ctx, layout, want_t):
    import torch

    from maria_amd import downsample, hwp
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    q, n_taps = 8, 161
    T_out = 2 * hwp.TILE_OUTPUTS + 67
    T = q * T_out - 3
    assert downsample.output_length(T, q) == T_out
    per_row = -(-T_out // hwp.TILE_OUTPUTS)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    x, c, ht, hp, want, tols = demodulate_case(D, T, q, n_taps)
    xbuf, xv, ld_x = place(x, layout, -3.0)
    d_c, d_ht, d_hp = on_device(c), on_device(ht), on_device(hp)
    before = xbuf.clone(), d_c.clone()
    ld_y = []

    def fresh():
        outs = []
        for _ in range(3):
            buf, view, ld = place(np.full((D, T_out), 7.0, np.float32), layout, 7.0)
            outs.append((buf, view))
        ld_y.append(ld)
        return outs

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_demodulate", ptr(xv[lo:hi]), ld_x, hi - lo, T, q, ptr(d_c), ptr(d_ht) if want_t else None, ptr(d_hp), n_taps,
                     ptr(outs[0][lo:hi]) if want_t else None, ptr(outs[1][lo:hi]), ptr(outs[2][lo:hi]), ld_y[0])

    outs = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before[0]) and torch.equal(d_c, before[1]), "an input changed"
    for k, name in enumerate("TQU"):
        buf, view = outs[k]
        if k or want_t:
            worst = float((np.abs(view.cpu().numpy().astype(np.float64) - want[k]) / tols[k]).max())
            print(f"{layout} {name}: max |y - ref| / tolerance = {worst:.3f}")
            assert worst <= 1.0, name
            view.fill_(7.0)
        assert bool((buf == 7.0).all()), "written outside the outputs"


@functools.lru_cache(maxsize=None)
def modulate_case(D):
    import hwp_ref as ref

    from maria_amd import hwp

    rng = np.random.default_rng(D)
    si, sc, ss = ((rng.standard_normal((D, T3)) * k).astype(np.float32) for k in (3.0, 1e-2, 1e-2))
    c = hwp.carrier(rng.uniform(0, 2 * np.pi, T3))
    want = ref.modulate(si, sc, ss, c)
    tol = 2.0**-24 * (np.abs(si) + np.abs(sc) + np.abs(ss)) * (1 + 1e-6)
    for a in (si, sc, ss, c, want, tol):
        a.setflags(write=False)
    return si, sc, ss, c, want, tol


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_hwp_modulate(gpu_ctx, layout, in_place):
    """Within 2^-24 (|i| + |c| + |s|) of the float64 expression (test_gpu_hwp.test_modulate_against_numpy's bound)."""
    import torch

    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // TILE)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    si, sc, ss, c, want, tol = modulate_case(D)
    (bi, vi, ld_in), (bc, vc, _), (bs, vs, _) = (place(a, layout, -3.0) for a in (si, sc, ss))
    d_c = on_device(c)
    before = [b.clone() for b in (bi, bc, bs)]
    fill = -3.0 if in_place else 7.0

    def fresh():
        buf, view, _ = place(si if in_place else np.full(si.shape, 7.0, np.float32), layout, fill)
        return [(buf, view)]

    def launch(lo, hi, outs):
        src = outs[0] if in_place else vi
        gpu_ctx.call("mrx_tod_hwp_modulate", ptr(src[lo:hi]), ptr(vc[lo:hi]), ptr(vs[lo:hi]), ld_in, hi - lo, T3, ptr(d_c), ptr(outs[0][lo:hi]), ld_in)

    ((obuf, ov),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert all(torch.equal(a, b) for a, b in zip((bi, bc, bs), before)), "an input changed"
    got = ov.cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol)
    assert untouched_outside(obuf, ov, fill), "written outside the rows"


# ---- mrx_timeconst.hip ----

@functools.lru_cache(maxsize=None)
def inverse_case(D, T):
    """3 N(0, 1) + 5 with timeconst_ref.POLES in rotation (a = 0: the copied rows), and the reference with ``init``."""
    import timeconst_ref as ref

    rng = np.random.default_rng(D + T)
    y = rng.standard_normal((D, T), dtype=np.float32)
    y *= np.float32(3.0)
    y += np.float32(5.0)
    a = np.asarray(ref.POLES)[np.arange(D) % len(ref.POLES)].copy()
    want = np.concatenate([ref.inverse(y[lo:lo + 256], a[lo:lo + 256], 1) for lo in range(0, D, 256)])
    for v in (y, a, want):
        v.setflags(write=False)
    return y, a, want


def run_inverse(gpu_ctx, D, T, per_row, layout, in_place):
    import torch

    from maria_amd._lib import ptr

    n_cu = resident(gpu_ctx)[0]
    y, a, want = inverse_case(D, T)
    ybuf, yv, ld = place(y, layout, -3.0)
    before = ybuf.clone()
    d_a = on_device(a)
    fill = -3.0 if in_place else 7.0

    def fresh():
        if in_place:
            buf, view, _ = place(y, layout, fill)
        else:
            buf, view, _ = place(np.empty((D, T), np.float32), layout, fill)
            view.fill_(fill)
        return [(buf, view)]

    def launch(lo, hi, outs):
        src = outs[0] if in_place else yv
        gpu_ctx.call("mrx_tod_onepole_inverse", ptr(src[lo:hi]), ld, hi - lo, T, ptr(d_a[lo:hi]), 1, ptr(outs[0][lo:hi]), ld)

    ((xbuf, xv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(ybuf, before), "the input changed"
    got = xv.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert untouched_outside(xbuf, xv, fill), "written outside the rows"


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_onepole_inverse_one_chunk_a_row(gpu_ctx, layout, in_place):
    """Rows of two tiles, one work item each: the slot parity and the copied rows' ``continue`` over three trips."""
    n_cu, R, need = resident(gpu_ctx)
    T = TILE + 5
    assert -(-T // TILE) <= CHUNK_TILES
    D = need
    strides(D, need)
    run_inverse(gpu_ctx, D, T, 1, layout, in_place)


def test_onepole_inverse_two_chunks_a_row(gpu_ctx):
    """Out of place, rows of 17 tiles: two work items a row, so that the read of the sample in front of a chunk happens
    on later trips too.  (About 170 MB a buffer.)"""
    n_cu, R, need = resident(gpu_ctx)
    T = CHUNK_TILES * TILE + 5
    per_row = -(-(-(-T // TILE)) // CHUNK_TILES)
    assert per_row == 2
    D = R + R // 4 + 1
    strides(D * per_row, need)
    run_inverse(gpu_ctx, D, T, per_row, "aligned", False)


# ---- mrx_regress.hip ----

@pytest.mark.parametrize("exact", [True, False])
def test_column_mean(gpu_ctx, exact):
    """Sixteen groups (the entry's most) of two rows each, one of them empty, two rows in none; the items come from the time
    axis.  exact: small integers with flags, a model and offsets at odd pitches, bit for bit; else Gaussian rows at aligned
    pitches within test_gpu_regress.mean_case's bounds.  The one-trip calls are blocks of columns."""
    import regress_ref as ref
    import torch
    from test_gpu_regress import EPS, rows

    from maria_amd import regress
    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    G = regress.MAX_GROUPS
    tiles = -(-need // G)
    T = tiles * TILE - 7
    strides(G * tiles, need)
    empty = 5
    groups = np.array([g for g in range(G) if g != empty] * 2 + [-1, G], np.int32)
    np.random.default_rng(3).shuffle(groups)
    D = groups.size
    x, model, flags, u, v, off = rows(D, T, 11 + exact, exact)
    flags[D - 1, :] = 2
    flags[groups == 0, 12345] = 1  # a sample flagged in every row of a group
    layout = "odd" if exact else "aligned"
    (xbuf, xv, ld_x), (mbuf, mv, ld_m), (fbuf, fv, ld_f) = place(x, layout, -3.0), place(model, layout, -5.0), place(flags, layout, 9)
    before = [b.clone() for b in (xbuf, mbuf, fbuf)]
    d_g, d_u, d_v, d_off = on_device(groups), on_device(u), on_device(v), on_device(off)

    def launch(c0, c1, S, W, mean, ld_c):
        gpu_ctx.call("mrx_tod_column_mean", ptr(xv[:, c0:c1]), ld_x, ptr(mv[:, c0:c1]) if exact else None, ld_m,
                     ptr(fv[:, c0:c1]) if exact else None, ld_f, D, c1 - c0, ptr(d_g), G, ptr(d_u), ptr(d_v), ptr(d_off) if exact else None,
                     ptr(S), ptr(W), ptr(mean), ld_c)

    def outputs(Tc):
        return (torch.full((G, Tc), 7.0, dtype=torch.float64, device=DEV), torch.full((G, Tc), 7.0, dtype=torch.float64, device=DEV),
                torch.full((G, Tc + 3), 7.0, dtype=torch.float32, device=DEV))

    big, again, small = outputs(T), outputs(T), outputs(T)
    launch(0, T, *big, T + 3)
    launch(0, T, *again, T + 3)
    step = max(1, n_cu // G) * TILE
    for c0 in range(0, T, step):
        c1 = min(T, c0 + step)
        S, W, mean = outputs(c1 - c0)
        launch(c0, c1, S, W, mean, c1 - c0 + 3)
        small[0][:, c0:c1], small[1][:, c0:c1], small[2][:, c0:c1] = S, W, mean[:, :c1 - c0]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((xbuf, mbuf, fbuf), before)), "an input changed"
    for k, name in enumerate(("S", "W", "mean")):
        assert torch.equal(big[k], again[k]), f"{name}: a second identical call gives other bits"
        assert torch.equal(big[k], small[k]), f"{name}: {int((big[k] != small[k]).sum())} elements differ from the one-trip calls"
    assert bool((big[2][:, T:] == 7.0).all()), "written outside the rows"
    S_got, W_got, m_got = big[0].cpu().numpy(), big[1].cpu().numpy(), big[2][:, :T].cpu().numpy()
    kw = dict(off=off, flags=flags, model=model) if exact else {}
    S_ref, W_ref, m_ref, A_ref = ref.column_mean(x, u, v, groups=groups, n_groups=G, **kw)
    assert not W_ref[empty].any() and W_ref[0].any()
    if exact:
        assert np.array_equal(bits(S_got), bits(S_ref)) and np.array_equal(bits(W_got), bits(W_ref)) and np.array_equal(bits(m_got), bits(m_ref))
        return
    bS, bW = D * EPS * A_ref, D * EPS * W_ref
    assert np.all(np.abs(S_got - S_ref) <= bS) and np.all(np.abs(W_got - W_ref) <= bW)
    ok = W_ref > 0
    q = np.where(ok, S_ref / np.where(ok, W_ref, 1), 0.0)
    carried = (bS + np.abs(q) * bW) / np.where(ok, W_ref - bW, 1)
    assert np.all(np.abs(m_got.astype(np.float64) - q) <= 2.0**-23 * np.abs(q) + carried)
    assert not m_got[~ok].any()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_regress_apply(gpu_ctx, layout, in_place):
    import regress_ref as ref
    import torch

    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // TILE)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    G, K, sign = 2, 5, 1 if in_place else -1
    rng = np.random.default_rng(D + K)
    x = (rng.standard_normal((D, T3)) * 3 + 5).astype(np.float32)
    B = rng.standard_normal((G, K, T3)).astype(np.float32)
    a = rng.standard_normal((D, K))
    groups = rng.integers(-1, G, D).astype(np.int32)
    groups[:2] = [-1, 1]
    want = ref.apply(x, B, a, groups=groups, sign=sign)
    assert np.array_equal(want[groups < 0], x[groups < 0])
    xbuf, xv, ld_x = place(x, layout, -3.0)
    bbuf, bv, ld_b = place(B.reshape(G * K, T3), layout, -7.0)
    before = xbuf.clone(), bbuf.clone()
    d_a, d_g = on_device(a), on_device(groups)
    fill = -3.0 if in_place else 7.0

    def fresh():
        buf, view, _ = place(x if in_place else np.full(x.shape, 7.0, np.float32), layout, fill)
        return [(buf, view)]

    def launch(lo, hi, outs):
        src = outs[0] if in_place else xv
        gpu_ctx.call("mrx_tod_regress_apply", ptr(src[lo:hi]), ld_x, hi - lo, T3, ptr(d_g[lo:hi]), G, ptr(bv), ld_b, K, ptr(d_a[lo:hi]), sign,
                     ptr(outs[0][lo:hi]), ld_x)

    ((ybuf, yv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before[0]) and torch.equal(bbuf, before[1]), "an input changed"
    got = yv.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert untouched_outside(ybuf, yv, fill), "written outside the rows"


# ---- mrx_ground.hip ----

@pytest.mark.parametrize("variant", ["flags, model, min_hits 8, keys of -1, odd pitches", "plain"])
def test_bin_reduce(gpu_ctx, variant):
    """Eleven bins: three workgroups a row, the last wave of the third with no bin (its ``continue``); the first bins hold 0,
    1, 63, 64, 65 and 129 samples (test_gpu_ground.keys).  Small integers: sums, hits and templates bit for bit."""
    import ground_ref as ref
    import torch
    from test_gpu_ground import SIZES, keys, rows

    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    K, T = 11, 64 * 11 + 5
    per_row = -(-K // WAVES)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    on = variant != "plain"
    min_hits = 8 if on else 1
    b = keys(T, K, D, absent=on)
    assert np.bincount(b[b >= 0], minlength=K)[:6].tolist() == SIZES
    x, model, flags = rows(D, T, D + on, exact=True)
    flags[D - 1, b == K - 1] = 2  # one row with a whole bin flagged
    order = np.argsort(b, kind="stable")
    order = order[b[order] >= 0].astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(b[b >= 0], minlength=K))]).astype(np.int32)
    layout = "odd" if on else "aligned"
    (xbuf, xv, ld_x), (mbuf, mv, ld_m), (fbuf, fv, ld_f) = place(x, layout, -3.0), place(model, layout, -5.0), place(flags, layout, 9)
    before = [v.clone() for v in (xbuf, mbuf, fbuf)]
    d_order, d_start = on_device(order), on_device(start)

    def fresh():
        outs = (torch.full((D, K), 7.0, dtype=torch.float64, device=DEV), torch.full((D, K), 12345, dtype=torch.int32, device=DEV),
                torch.full((D, K), 7.0, dtype=torch.float32, device=DEV))
        return [(o, o) for o in outs]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_bin_reduce", ptr(xv[lo:hi]), ld_x, ptr(mv[lo:hi]) if on else None, ld_m, ptr(fv[lo:hi]) if on else None, ld_f,
                     hi - lo, T, ptr(d_order), order.size, ptr(d_start), K, min_hits, ptr(outs[0][lo:hi]), ptr(outs[1][lo:hi]), ptr(outs[2][lo:hi]))

    (sums, _), (hits, _), (tmpl, _) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert all(torch.equal(a, c) for a, c in zip((xbuf, mbuf, fbuf), before)), "an input changed"
    s_ref, h_ref, t_ref, _ = ref.bin_reduce(x, b, K, flags=flags if on else None, model=model if on else None, min_hits=min_hits)
    assert not on or h_ref[D - 1, K - 1] == 0
    assert np.array_equal(hits.cpu().numpy(), h_ref)
    assert np.array_equal(bits(sums.cpu().numpy()), bits(s_ref)) and np.array_equal(bits(tmpl.cpu().numpy()), bits(t_ref))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bin_apply(gpu_ctx, layout, in_place):
    import ground_ref as ref
    import torch

    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // TILE)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    K, sign = 360, 1 if in_place else -1
    rng = np.random.default_rng(D + K)
    x = (rng.standard_normal((D, T3)) * 3 + 5).astype(np.float32)
    tmpl = rng.standard_normal((D, K)).astype(np.float32)
    b = rng.integers(-1, K + 1, T3).astype(np.int32)  # -1 and K: in no bin
    want = ref.bin_apply(x, b, tmpl, sign)
    assert np.array_equal(want[:, b == K], x[:, b == K]) and (b == -1).any()
    xbuf, xv, ld_x = place(x, layout, -3.0)
    before = xbuf.clone()
    d_b, d_t = on_device(b), on_device(tmpl)
    fill = -3.0 if in_place else 7.0

    def fresh():
        buf, view, _ = place(x if in_place else np.full(x.shape, 7.0, np.float32), layout, fill)
        return [(buf, view)]

    def launch(lo, hi, outs):
        src = outs[0] if in_place else xv
        gpu_ctx.call("mrx_tod_bin_apply", ptr(src[lo:hi]), ld_x, hi - lo, T3, ptr(d_b), ptr(d_t[lo:hi]), K, sign, ptr(outs[0][lo:hi]), ld_x)

    ((ybuf, yv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before), "the input changed"
    got = yv.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert untouched_outside(ybuf, yv, fill), "written outside the rows"


# ---- mrx_subscan.hip, mrx_stats.hip ----

SEGMENT_LENGTHS = [0, 1, 63, 64, 65, 2, 129, 37, 128, 5, 200, 3, 127, 90, 256, 17]  # uneven, about 64 a segment


def wave_shape(gpu_ctx):
    """(n_cu, R, D, S, T, bounds, the workgroups): D rows of S segments, one (row, segment) a wave and four a workgroup, so
    that the workgroups number at least 2 R + R / 2 + 1; samples in no segment at both ends of a row."""
    n_cu, R, need = resident(gpu_ctx)
    D = rows_for(need, 3)
    S = -(-WAVES * need // D)
    assert S <= len(SEGMENT_LENGTHS)
    n_groups = (D * S + WAVES - 1) // WAVES
    strides(n_groups, need)
    bounds = (2 + np.concatenate([[0], np.cumsum(SEGMENT_LENGTHS[:S])])).astype(np.int32)
    assert {0, 1, 63, 64, 65} <= set(np.diff(bounds).tolist())
    return n_cu, R, D, S, int(bounds[-1]) + 3, bounds, n_groups


def wave_rows(D, S, n_groups, R):
    return traced_rows(D, n_groups, R, lambda w: [(WAVES * w + k) // S for k in range(WAVES)])


@pytest.mark.parametrize("variant", ["flags and a model, K 3, odd pitches", "plain, K 1, small integers"])
def test_segment_normal(gpu_ctx, variant):
    """K = 3 on Gaussian rows within (L + 1) 2^-53 sum|terms| of the reference's fsum, hits exact; K = 1 on small integers
    bit for bit.  The reference (loops and fsum a pair) runs on traced_rows' subset, the one-trip comparison on every row."""
    import subscans_ref as ref
    import torch
    from test_gpu_subscans import HALF_ULP, rows

    from maria_amd._lib import ptr

    n_cu, R, D, S, T, bounds, n_groups = wave_shape(gpu_ctx)
    on = variant.startswith("flags")
    K = 3 if on else 1
    x, model, flags = rows(D, T, D + on, exact=not on)
    flags[D - 1, bounds[2]:bounds[3]] = 2  # one segment wholly flagged in the last row
    layout = "odd" if on else "aligned"
    (xbuf, xv, ld_x), (mbuf, mv, ld_m), (fbuf, fv, ld_f) = place(x, layout, -3.0), place(model, layout, -5.0), place(flags, layout, 9)
    before = [v.clone() for v in (xbuf, mbuf, fbuf)]
    d_bound = on_device(bounds)

    def fresh():
        outs = (torch.full((D, S, K, K), 7.0, dtype=torch.float64, device=DEV), torch.full((D, S, K), 7.0, dtype=torch.float64, device=DEV),
                torch.full((D, S), 12345, dtype=torch.int32, device=DEV))
        return [(o, o) for o in outs]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_segment_normal", ptr(xv[lo:hi]), ld_x, ptr(mv[lo:hi]) if on else None, ld_m, ptr(fv[lo:hi]) if on else None, ld_f,
                     hi - lo, T, ptr(d_bound), S, K, ptr(outs[0][lo:hi]), ptr(outs[1][lo:hi]), ptr(outs[2][lo:hi]))

    (N, _), (r, _), (hits, _) = three_ways(launch, fresh, D, max(1, WAVES * n_cu // S))
    assert all(torch.equal(a, c) for a, c in zip((xbuf, mbuf, fbuf), before)), "an input changed"
    sub = wave_rows(D, S, n_groups, R)
    print(f"the loop reference runs on {sub.size} of {D} rows ({sub.size / D:.1%})")
    N_got, r_got, h_got = N.cpu().numpy()[sub], r.cpu().numpy()[sub], hits.cpu().numpy()[sub]
    N_ref, r_ref, h_ref, aN, ar = ref.normal_equations(x[sub], bounds, K, flags=flags[sub] if on else None, model=model[sub] if on else None)
    assert np.array_equal(h_got, h_ref)
    empty = np.diff(bounds) == 0
    assert not N_got[:, empty].any() and not r_got[:, empty].any() and (not on or h_ref[-1, 2] == 0)
    if not on:
        assert np.array_equal(bits(N_got), bits(N_ref)) and np.array_equal(bits(r_got), bits(r_ref))
        return
    L = np.diff(bounds).astype(np.float64)
    bN, br = (L[None, :, None, None] + 1) * HALF_ULP * aN, (L[None, :, None] + 1) * HALF_ULP * ar
    assert np.all(np.abs(N_got - N_ref) <= bN) and np.all(np.abs(r_got - r_ref) <= br)


@pytest.mark.parametrize("variant", ["flags and a model, odd pitches", "plain"])
def test_segment_moments(gpu_ctx, variant):
    """Counts, min and max exact, the sums within cuts_ref.bounds_of (test_gpu_cuts.moments_case's acceptance).  The
    reference (loops and fsum a pair) runs on traced_rows' subset, the one-trip comparison on every row."""
    import cuts_ref as ref
    import torch
    from test_gpu_subscans import rows

    from maria_amd._lib import ptr

    n_cu, R, D, S, T, bounds, n_groups = wave_shape(gpu_ctx)
    on = variant.startswith("flags")
    x, model, flags = rows(D, T, D + 7 + on, exact=False)
    flags[D - 1, bounds[2]:bounds[3]] = 2
    layout = "odd" if on else "aligned"
    (xbuf, xv, ld_x), (mbuf, mv, ld_m), (fbuf, fv, ld_f) = place(x, layout, -3.0), place(model, layout, -5.0), place(flags, layout, 9)
    before = [v.clone() for v in (xbuf, mbuf, fbuf)]
    d_bound = on_device(bounds)

    def fresh():
        outs = (torch.full((D, S, 8), 7.0, dtype=torch.float64, device=DEV), torch.full((D, S, 2), 12345, dtype=torch.int32, device=DEV))
        return [(o, o) for o in outs]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_segment_moments", ptr(xv[lo:hi]), ld_x, ptr(mv[lo:hi]) if on else None, ld_m, ptr(fv[lo:hi]) if on else None, ld_f,
                     hi - lo, T, ptr(d_bound), S, ptr(outs[0][lo:hi]), ptr(outs[1][lo:hi]))

    (stat, _), (count, _) = three_ways(launch, fresh, D, max(1, WAVES * n_cu // S))
    assert all(torch.equal(a, c) for a, c in zip((xbuf, mbuf, fbuf), before)), "an input changed"
    sub = wave_rows(D, S, n_groups, R)
    print(f"the loop reference runs on {sub.size} of {D} rows ({sub.size / D:.1%})")
    stat, count = stat.cpu().numpy()[sub], count.cpu().numpy()[sub]
    got = {name: stat[:, :, k] for k, name in enumerate(ref.NAMES)}
    got["hits"], got["pairs"] = count[:, :, 0], count[:, :, 1]
    assert not stat[:, :, 7].any()
    want = ref.moments(x[sub], bounds, flags=flags[sub] if on else None, model=model[sub] if on else None)
    for k in ("hits", "pairs", "min", "max"):
        assert np.array_equal(got[k], want[k]), k
    nothing = want["hits"] == 0
    assert nothing[:, np.diff(bounds) == 0].all() and (not on or nothing[-1, 2])
    for k in ref.NAMES:
        assert not got[k][nothing].any(), k
    for k, b in ref.bounds_of(want).items():
        err = np.abs(got[k] - want[k])
        print(f"{variant} {k}: max |got - ref| / bound = {(err / np.where(b > 0, b, 1)).max():.3g}")
        assert np.all(err <= b), k


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_segment_apply(gpu_ctx, layout, in_place):
    """Segments of test_gpu_subscans.LENGTHS (as many as fit a row): some cross tiles, some samples are in none."""
    import subscans_ref as ref
    import torch
    from test_gpu_subscans import make_bounds

    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    per_row = -(-T3 // TILE)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    K, sign = 4, 1 if in_place else -1
    rng = np.random.default_rng(D + K)
    x = (rng.standard_normal((D, T3)) * 3 + 5).astype(np.float32)
    bounds = make_bounds(T3, 4)
    S = len(bounds) - 1
    assert np.diff(bounds).max() > TILE and bounds[0] > 0 and bounds[-1] < T3
    a = rng.standard_normal((D, S, K))
    want = ref.apply(x, bounds, a, sign=sign)
    xbuf, xv, ld_x = place(x, layout, -3.0)
    before = xbuf.clone()
    d_a, d_bound = on_device(a), on_device(bounds)
    fill = -3.0 if in_place else 7.0

    def fresh():
        buf, view, _ = place(x if in_place else np.full(x.shape, 7.0, np.float32), layout, fill)
        return [(buf, view)]

    def launch(lo, hi, outs):
        src = outs[0] if in_place else xv
        gpu_ctx.call("mrx_tod_segment_apply", ptr(src[lo:hi]), ld_x, hi - lo, T3, ptr(d_bound), S, K, ptr(d_a[lo:hi]), sign, ptr(outs[0][lo:hi]), ld_x)

    ((ybuf, yv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    assert torch.equal(xbuf, before), "the input changed"
    got = yv.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert untouched_outside(ybuf, yv, fill), "written outside the rows"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_segment_flag(gpu_ctx, layout):
    """In place on the flags (the entry has no other form).  Every length of test_gpu_subscans.LENGTHS; the last tile of
    a row has no segment, and about half of the (row, segment) pairs are masked."""
    import cuts_ref as ref
    from test_gpu_subscans import LENGTHS, make_bounds

    from maria_amd._lib import ptr

    n_cu, R, need = resident(gpu_ctx)
    T = 2 * FLAG_TILE + 517
    per_row = -(-T // FLAG_TILE)
    D = rows_for(need, per_row)
    strides(D * per_row, need)
    value = 2
    rng = np.random.default_rng(D)
    bounds = make_bounds(T, 1)
    S = len(bounds) - 1
    assert S == len(LENGTHS) and bounds[-1] < 2 * FLAG_TILE
    old = ((rng.random((D, T)) < 0.1) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    mask = (rng.random((D, S)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (D, S)).astype(np.uint8)
    mask[D - 1] = 1
    mask[1] = 0
    want = ref.flag_segments(old, bounds, mask, value)
    d_mask, d_bound = on_device(mask), on_device(bounds)
    ld_f = []

    def fresh():
        buf, view, ld = place(old, layout, 9, wide=16)
        ld_f.append(ld)
        return [(buf, view)]

    def launch(lo, hi, outs):
        gpu_ctx.call("mrx_tod_segment_flag", ptr(outs[0][lo:hi]), ld_f[0], hi - lo, T, ptr(d_bound), S, ptr(d_mask[lo:hi]), value)

    ((fbuf, fv),) = three_ways(launch, fresh, D, max(1, n_cu // per_row))
    got = fv.cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert untouched_outside(fbuf, fv, 9), "written outside the rows"
