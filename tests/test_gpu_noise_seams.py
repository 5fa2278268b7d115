"""The GLS noise kernels at the seams of their streaming loops: mrx_tod_noise_filter,
mrx_tod_noise_filter_modes, mrx_tod_mode_project (mrx_nfilter.hip) and mrx_tod_welch (mrx_psd.hip).

These entries launch a plain grid (a workgroup a row, or a tile of samples), so their seams lie inside the workgroup.  The
filter walks its row in pairs of overlap-save blocks of L = N - 2 K outputs and hands the 2 K samples two pairs share from
one pair to the next in per-thread registers cy[0 .. KC - 1]; slot i of thread t holds carried sample v = i threads + t and
is live only where v < 2 K:

  route   K            N      threads   KC
  A       0 .. 512     4096   512       2
  B       513 .. 2048  8192   1024      4

The carry is used from the second pair on (T > P = 2 L).  tests/test_gpu_noise_filter.py reaches route A's second pair only at
K = 255 (slot 0 alone) and route B's only at K = 1024 and 2048 (full slots); here every K below runs at every T of
{L, L + 1, P - 1, P, P + 1, P + K, P + L, P + L + 1, 2 P, 2 P + 1, 3 P - 1}, where the pair count, the `s >= T` break and the
empty second block change over, with NaN in the padding of x and of sqrt_w:

  K      route   live carry slots (lanes of the last)
  0      A       none
  256    A       0 (all 512)
  257    A       0, 1 (2 lanes)
  511    A       0, 1 (510)
  512    A       0, 1 (all)
  513    B       0, 1 (2 lanes)
  1024   B       0, 1 (all 1024)
  1025   B       0, 1, 2 (2 lanes)
  1537   B       0 .. 3 (2 lanes)
  2047   B       0 .. 3 (1022)
  2048   B       0 .. 3 (all; L = 2 K)

Every test asserts its geometric preconditions on the host before it launches (three pairs at the longest T, the occupancy of
the slots it claims, D > 65535 x 32 for the strided row-group loop, scipy's segment count for the spectrum)."""

import numpy as np
import pytest
import scipy.signal
import test_gpu_noise_estimate as est
from test_gpu_noise_filter import ROW_TOL, _lags, _reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 7.0
SW_MODES = ("none", "shared", "rows")
PADS = (0, 1, 3)
TAIL = 64  # sentinel elements after the last row of an out-of-place output


def route(K):
    """(N, threads, KC, L, P) of mrx_tod_noise_filter at K lags (mrx_nfilter.hip)"""
    N, threads, KC = (4096, 512, 2) if K <= 512 else (8192, 1024, 4)
    L = N - 2 * K
    return N, threads, KC, L, 2 * L


def seam_lengths(K):
    _, _, _, L, P = route(K)
    return sorted({L, L + 1, P - 1, P, P + 1, P + K, P + L, P + L + 1, 2 * P, 2 * P + 1, 3 * P - 1})


def _dev(a, dtype):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _padded(a, ld, fill=np.nan):
    """[D, ld] float32 with a in its first columns and ``fill`` in the padding"""
    buf = np.full((a.shape[0], ld), fill, np.float32)
    buf[:, :a.shape[1]] = a
    return buf


def _sqrt_w(mode, D, T, ld, rng):
    """(host buffer or None, ld_w, the float64 factor [rows, T]): uniform on [0, 1.5) with a few exact zeros, NaN padding"""
    if mode == "none":
        return None, 0, np.ones((1, T))
    rows = 1 if mode == "shared" else D
    s = rng.uniform(0.0, 1.5, (rows, T)).astype(np.float32)
    s[:, rng.integers(0, T, 5)] = 0.0
    s[:, [0, T - 1]] = (0.0, 1.25) if mode == "shared" else (0.75, 0.0)
    return _padded(s, ld), (0 if mode == "shared" else ld), s.astype(np.float64)


def _seam_rows(T, K, L, rng):
    """noise times 3 on an offset of 50; noise; impulses of +-1 around every block edge and at both ends; all ones"""
    x = np.zeros((4, T), np.float32)
    x[0] = 3.0 * rng.normal(size=T) + 50.0
    x[1] = rng.normal(size=T)
    j = np.arange(T // L + 3)[:, None] * L
    pos = np.concatenate([(j + np.array([-K - 1, -K, -1, 0, K - 1, K])).ravel(), [0, T - 1]])
    pos = np.unique(pos[(pos >= 0) & (pos < T)])
    x[2, pos] = rng.choice([-1.0, 1.0], pos.size)
    x[3] = 1.0
    return x


def _filter(ctx, entry, xbuf, ld, T, k, sbuf, ld_w, in_place, extra=()):
    """One call of the plain or the modes filter on the host rows xbuf [D, ld].  Returns (the whole output buffer with
    its TAIL as a flat host array, x's buffer after the call)."""
    import torch

    from maria_amd._lib import ptr

    D = xbuf.shape[0]
    d_x = _dev(xbuf, np.float32)
    d_y = d_x if in_place else torch.full((D * ld + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    d_k = _dev(k, np.float64)
    d_s = None if sbuf is None else _dev(sbuf, np.float32)
    ctx.call(entry, ptr(d_x), ld, ptr(d_y), ld, D, T, ptr(d_k), k.shape[1] - 1, ptr(d_s), ld_w, *extra)
    torch.cuda.synchronize()
    return d_y.cpu().numpy().ravel(), d_x.cpu().numpy()


def _plain(ctx, xbuf, ld, T, k, sbuf, ld_w, in_place):
    return _filter(ctx, "mrx_tod_noise_filter", xbuf, ld, T, k, sbuf, ld_w, in_place)


def _with_modes(ctx, xbuf, ld, T, k, sbuf, ld_w, in_place, U, b):
    from maria_amd._lib import ptr

    d_U, d_b = _dev(U, np.float64), _dev(b, np.float32)  # (held until the call has synchronised)
    return _filter(ctx, "mrx_tod_noise_filter_modes", xbuf, ld, T, k, sbuf, ld_w, in_place, (ptr(d_U), U.shape[1], ptr(d_b)))


def _outside_untouched(flat, D, ld, T, what):
    """out of place: the sentinel stands in every row's padding and after the last row"""
    body = flat[:D * ld].reshape(D, ld)
    assert np.all(body[:, T:] == SENTINEL), f"{what}: written past T inside a row's pitch"
    assert np.all(flat[D * ld:] == SENTINEL), f"{what}: written after the last row"
    return body[:, :T]


# ---- A. mrx_tod_noise_filter on its seams --------------------------------------------------------------------------

SEAM_K = [  # K, the carry slots the case claims
    (0, ()),
    (256, (0,)),
    (257, (0, 1)),
    (511, (0, 1)),
    (512, (0, 1)),
    (513, (0, 1)),
    (1024, (0, 1)),
    (1025, (0, 1, 2)),
    (1537, (0, 1, 2, 3)),
    (2047, (0, 1, 2, 3)),
    (2048, (0, 1, 2, 3)),
]


@pytest.mark.parametrize("K,slots", SEAM_K)
def test_filter_on_its_seams(gpu_ctx, K, slots):
    """Per K every T of seam_lengths(K) on four rows (D = 4), sqrt_w none / shared / per row and the pitch T + 0 / 1 / 3
    going round with T, NaN in every padding:
      1. out of place against the float64 convolution, per row within ROW_TOL = 2e-6 of max(|k| * |s x|);
      2. in place: the bits of 1;  3. a second identical call: the bits of 1;
      4. out of place the sentinel past T and after the rows stands and x is unchanged; in place x's padding is unchanged.
    Worst row error measured on an MI355X, K 0 / 256 / 257 / 511 / 512 / 513 / 1024 / 1025 / 1537 / 2047 / 2048:
    4.7e-7 / 3.6e-7 / 3.4e-7 / 4.0e-7 / 4.2e-7 / 4.6e-7 / 3.8e-7 / 4.0e-7 / 4.0e-7 / 3.9e-7 / 3.8e-7."""
    N, threads, KC, L, P = route(K)
    lengths = seam_lengths(K)
    n_pairs = -(-lengths[-1] // P)
    assert n_pairs >= 3, f"K {K}: the longest T {lengths[-1]} gives {n_pairs} pairs of {P} outputs, below three"
    assert L >= 2 * K and L >= 1, f"K {K}: L {L} is below 2 K, outside what the kernel accepts"
    live = tuple(i for i in range(KC) if 2 * K > i * threads)
    assert slots == live, f"K {K}: the case claims carry slots {slots}, but 2 K = {2 * K} > i x {threads} holds for {live}"
    rng = np.random.default_rng(1000 + K)
    k = _lags(4, K, rng)
    worst = (0.0, None)
    for i, T in enumerate(lengths):
        ld = T + PADS[(i + i // 3) % 3]
        mode = SW_MODES[i % 3]
        x = _seam_rows(T, K, L, rng)
        xbuf = _padded(x, ld)
        sbuf, ld_w, s = _sqrt_w(mode, 4, T, ld, rng)
        what = f"K {K} T {T} (L {L}, P {P}) ld {ld} sqrt_w {mode}"
        flat, x_after = _plain(gpu_ctx, xbuf, ld, T, k, sbuf, ld_w, False)
        got = _outside_untouched(flat, 4, ld, T, what)
        assert np.array_equal(_bits(x_after), _bits(xbuf)), f"{what}: out of place changed x"
        ref, mag = _reference(x, k, s)
        diff = np.abs(got - ref)
        err = diff.max(axis=1) / np.maximum(mag, 1e-300)
        if not err.max() <= ROW_TOL:  # (a NaN fails too)
            d = int(np.nanargmax(np.where(np.isfinite(err), err, np.inf)))
            t = int(np.nanargmax(np.where(np.isfinite(diff[d]), diff[d], np.inf)))
            seam = int(min(t % L, L - t % L))
            print(f"{what}: row {d} error {err[d]:.2e} at sample {t}, {seam} from a multiple of L, block {t // L}")
        assert err.max() <= ROW_TOL, (what, err.tolist())
        if err.max() > worst[0]:
            worst = (float(err.max()), (T, int(err.argmax()), mode))
        again, _ = _plain(gpu_ctx, xbuf, ld, T, k, sbuf, ld_w, False)
        assert np.array_equal(_bits(again), _bits(flat)), f"{what}: a second identical call gives other bits"
        _, y_in = _plain(gpu_ctx, xbuf, ld, T, k, sbuf, ld_w, True)
        differ = np.flatnonzero((_bits(y_in[:, :T]) != _bits(got)).any(axis=0))
        assert differ.size == 0, (f"{what}: in place differs from out of place at {differ.size} samples, the first {int(differ[0])}, "
                                  f"{int(min(differ[0] % L, L - differ[0] % L))} from a multiple of L")
        assert np.array_equal(_bits(y_in[:, T:]), _bits(xbuf[:, T:])), f"{what}: in place wrote into the padding"
    print(f"seams K {K} route {'A' if N == 4096 else 'B'} slots {slots}: worst row error {worst[0]:.2e} of max(|k| * |s x|) at "
          f"(T, row, sqrt_w) {worst[1]} over T {lengths}")


@pytest.mark.parametrize("K", [257, 512, 513])
def test_filter_with_zero_modes_on_the_seams_is_the_plain_filter(gpu_ctx, K):
    """mrx_tod_noise_filter_modes with m = 3 and U = 0 at T = P + 1 (out of place) and 2 P + 1 (in place): the subtraction
    leaves x as it is and the filter then runs in place on the output, so the plain filter's bits"""
    N, threads, KC, L, P = route(K)
    assert 2 * K > threads, f"K {K}: carry slot 1 is not live"
    rng = np.random.default_rng(2000 + K)
    k = _lags(4, K, rng)
    for i, (T, in_place) in enumerate(((P + 1, False), (2 * P + 1, True))):
        assert T > P, "one pair only: the carry is not used"
        ld = T + PADS[1 + i]
        x = _seam_rows(T, K, L, rng)
        xbuf = _padded(x, ld)
        sbuf, ld_w, _ = _sqrt_w(SW_MODES[1 + i], 4, T, ld, rng)
        b = rng.normal(size=(3, T)) * 3.0
        flat, _ = _plain(gpu_ctx, xbuf, ld, T, k, sbuf, ld_w, False)
        plain = _outside_untouched(flat, 4, ld, T, (K, T))
        out, _ = _with_modes(gpu_ctx, xbuf, ld, T, k, sbuf, ld_w, in_place, np.zeros((4, 3)), b)
        if in_place:
            got = out.reshape(4, ld)
            assert np.array_equal(_bits(got[:, T:]), _bits(xbuf[:, T:])), f"K {K} T {T}: in place wrote into the padding"
            got = got[:, :T]
        else:
            got = _outside_untouched(out, 4, ld, T, (K, T, "modes"))
        assert np.array_equal(_bits(got), _bits(plain)), f"K {K} T {T}: {(got != plain).sum()} samples differ from the plain filter"


# ---- B1, B2. mrx_tod_noise_filter_modes: the subtraction's tiles (256 samples x 32 rows) and its row-group loop -------

def _modes_acceptance(x, U, b, k, s):
    """the float64 filter of x - U b, and per row max(|k| * |s| (|x| + |U||b|)) (test_gpu_noise_modes.py's acceptance)"""
    b64 = b.astype(np.float64)
    ref, _ = _reference(x.astype(np.float64) - U @ b64, k, s)
    _, mag = _reference(np.abs(x).astype(np.float64) + np.abs(U) @ np.abs(b64), k, s)
    return ref, mag


@pytest.mark.parametrize("D", [31, 32, 33, 65])
def test_filter_with_modes_on_the_subtraction_tile_edges(gpu_ctx, D):
    """T 255, 256, 257, 513 x m 1, 16 at K = 16, in place and out of place, NaN in the padding of x and sqrt_w"""
    K = 16
    rng = np.random.default_rng(3000 + D)
    k = _lags(D, K, rng)
    worst = 0.0
    for i, (T, m) in enumerate((T, m) for T in (255, 256, 257, 513) for m in (1, 16)):
        ld = T + PADS[i % 3]
        x = (rng.normal(size=(D, T)) * rng.uniform(0.1, 10.0, (D, 1))).astype(np.float32)
        x[0] += 50.0
        xbuf = _padded(x, ld)
        U = rng.normal(size=(D, m))
        b = (rng.normal(size=(m, T)) * 3.0).astype(np.float32)
        sbuf, ld_w, s = _sqrt_w(SW_MODES[(i + i // 3) % 3], D, T, ld, rng)
        ref, mag = _modes_acceptance(x, U, b, k, s)
        what = f"modes filter D {D} T {T} m {m} ld {ld}"
        flat, x_after = _with_modes(gpu_ctx, xbuf, ld, T, k, sbuf, ld_w, False, U, b)
        got = _outside_untouched(flat, D, ld, T, what)
        assert np.array_equal(_bits(x_after), _bits(xbuf)), f"{what}: out of place changed x"
        err = np.abs(got - ref).max(axis=1) / np.maximum(mag, 1e-300)
        assert err.max() <= ROW_TOL, (what, float(err.max()), int(err.argmax()))
        worst = max(worst, float(err.max()))
        _, y_in = _with_modes(gpu_ctx, xbuf, ld, T, k, sbuf, ld_w, True, U, b)
        assert np.array_equal(_bits(y_in[:, :T]), _bits(got)), f"{what}: in place differs from out of place"
        assert np.array_equal(_bits(y_in[:, T:]), _bits(xbuf[:, T:])), f"{what}: in place wrote into the padding"
    print(f"modes filter tile edges D {D}: worst row error {worst:.2e}")


def test_filter_with_modes_goes_round_its_row_group_loop(gpu_ctx):
    """D = 65535 x 32 + 33 rows of T = 3, K = 0, m = 1, in place: the subtraction's grid has 65535 row groups of 32 rows, so
    the last 33 rows are the second trip of groups 0 and 1.  Against k0[d] (x - U b) in float64, every row."""
    import torch

    from maria_amd._lib import ptr

    D, T, ld = 65535 * 32 + 33, 3, 4
    assert D > 65535 * 32, f"D {D}: the row-group loop makes one trip only"
    rng = np.random.default_rng(4000)
    x = (rng.normal(size=(D, T)) * 4.0).astype(np.float32)
    xbuf = _padded(x, ld)
    U = rng.normal(size=(D, 1))
    b = (rng.normal(size=(1, T)) * 3.0).astype(np.float32)
    k0 = rng.normal(size=(D, 1))
    d_x, d_k, d_U, d_b = _dev(xbuf, np.float32), _dev(k0, np.float64), _dev(U, np.float64), _dev(b, np.float32)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    gpu_ctx.call("mrx_tod_noise_filter_modes", ptr(d_x), ld, ptr(d_x), ld, D, T, ptr(d_k), 0, None, 0, ptr(d_U), 1, ptr(d_b))
    stop.record()
    torch.cuda.synchronize()
    y = d_x.cpu().numpy()
    b64 = b.astype(np.float64)
    ref = k0 * (x.astype(np.float64) - U * b64)
    mag = (np.abs(k0) * (np.abs(x).astype(np.float64) + np.abs(U) * np.abs(b64))).max(axis=1)
    err = np.abs(y[:, :T] - ref).max(axis=1) / np.maximum(mag, 1e-300)
    bad = np.flatnonzero(~(err <= ROW_TOL))
    print(f"row-group loop D {D}: worst row error {np.nanmax(err):.2e}, {start.elapsed_time(stop):.1f} ms on the device")
    assert bad.size == 0, f"{bad.size} rows wrong, the first {int(bad[0])} (row group {int(bad[0]) // 32}): error {err[bad[0]]:.2e}"
    assert np.isnan(y[:, T:]).all(), "in place wrote into the padding"


# ---- B3. mrx_tod_mode_project: every tail of its four-rows-a-wave loop ----------------------------------------------

PROJECT_T = (63, 64, 65, 127, 128, 129, 257)
PROJECT_M = (1, 4, 8, 9, 16)
PROJECT_FULL = (3, 16, 19, 26, 35)  # no main trip; a main trip and no tail; tails of 1, 1, 1, 0 / 3, 3, 2, 2 / 1, 1, 1, 0 rows


def _project_cases(D):
    if D in PROJECT_FULL:
        return [(T, m) for T in PROJECT_T for m in PROJECT_M]
    return [(PROJECT_T[D % 7], PROJECT_M[D % 5]), (PROJECT_T[(D + 3) % 7], PROJECT_M[(D + 2) % 5])]


def test_mode_project_cases_cover_the_tails():
    """(host arithmetic only) D = 1 .. 35 gives every wave every tail of 0 .. 3 rows with and without a main trip"""
    seen = set()
    for D in range(1, 36):
        for w in range(4):
            rows = len(range(w, D, 4))
            seen.add((rows // 4 > 0, rows % 4))
    assert seen == {(main, tail) for main in (False, True) for tail in range(4)}, seen
    for D in PROJECT_FULL:
        assert set(_project_cases(D)) == {(T, m) for T in PROJECT_T for m in PROJECT_M}
    assert {T for D in range(1, 36) for T, _ in _project_cases(D)} == set(PROJECT_T)


@pytest.mark.parametrize("D", range(1, 36))
def test_mode_project_on_every_tail(gpu_ctx, D):
    """a = U^T x against float64 numpy within 1e-13 of sum_d |U| |x| per sample, NaN in x's padding, the output prefilled;
    a second call gives the same bits"""
    import torch

    from maria_amd._lib import ptr

    rng = np.random.default_rng(5000 + D)
    worst = 0.0
    for i, (T, m) in enumerate(_project_cases(D)):
        ld = T + PADS[i % 3]
        x = (rng.normal(size=(D, T)) * rng.uniform(0.1, 10.0, (D, 1)) + 3.0).astype(np.float32)
        U = rng.normal(size=(D, m))
        d_x, d_U = _dev(_padded(x, ld), np.float32), _dev(U, np.float64)
        outs = []
        for _ in range(2):
            a = torch.full((m * T + TAIL,), SENTINEL, dtype=torch.float64, device=DEV)
            gpu_ctx.call("mrx_tod_mode_project", ptr(d_x), ld, D, T, ptr(d_U), m, ptr(a))
            torch.cuda.synchronize()
            outs.append(a.cpu().numpy())
        what = f"mode project D {D} T {T} m {m} ld {ld}"
        assert np.all(outs[0][m * T:] == SENTINEL), f"{what}: written after the output"
        assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), f"{what}: a second call gives other bits"
        xs = x.astype(np.float64)
        ref, mag = U.T @ xs, np.abs(U).T @ np.abs(xs)
        err = np.abs(outs[0][:m * T].reshape(m, T) - ref) / mag
        assert err.max() <= 1e-13, (what, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))
        worst = max(worst, float(err.max()))
    print(f"mode project D {D}: worst error {worst:.1e} of sum |U| |x|")


# ---- B4. mrx_tod_welch: every residue of the segment count modulo a batch ------------------------------------------

@pytest.mark.parametrize("nperseg", est.LENGTHS)
def test_welch_on_its_batch_edges(gpu_ctx, nperseg):
    """A batch holds G pairs of segments (G nperseg >= 2048): nseg = 2, 3, 2 G - 1 .. 2 G + 2, 4 G, 4 G + 1, the row ending
    on the last segment or h - 1 samples after it; pitch T + 67, NaN in the padding.  test_gpu_noise_estimate's acceptance."""
    G, h, fs = max(1, 2048 // nperseg), nperseg // 2, 37.0
    rng = np.random.default_rng(6000 + nperseg)
    for nseg in sorted(n for n in {2, 3, 2 * G - 1, 2 * G, 2 * G + 1, 2 * G + 2, 4 * G, 4 * G + 1} if n >= 1):
        for r in (0, h - 1):
            T = (nseg - 1) * h + nperseg + r
            rows = est._rows(T, fs, nperseg, rng)
            n_scipy = scipy.signal.spectrogram(rows[0].astype(np.float64), fs, nperseg=nperseg, noverlap=h)[1].size
            assert n_scipy == nseg, f"nperseg {nperseg} T {T}: scipy takes {n_scipy} segments, the case claims {nseg}"
            got = est._welch(gpu_ctx, _dev(_padded(rows, T + 67), np.float32), T, nperseg, fs)
            ref = est._reference(rows, fs, nperseg)
            est._check(got, ref, (nperseg, nseg, T))
            top = np.abs(ref).max(axis=1, keepdims=True)
            print(f"welch nperseg {nperseg} nseg {nseg} T {T}: worst row error {(np.abs(got - ref) / top).max():.2e} of the row's max")
