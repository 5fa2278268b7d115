"""The two TOD kernels of mrx_tod.hip on their own, row by row against float64 scipy / numpy:
mrx_sosfilt at every cascade length, across the chunk kernel's workgroups (65 536 samples) and
the scan kernel's blocks (256 detectors), in the layouts the callers use; and
mrx_tod_detrend_window against numpy's own in-place float32 arithmetic."""

import ctypes as C

import numpy as np
import pytest
import scipy.signal

pytestmark = pytest.mark.gpu

FS = 400.0
SENTINEL = -1234.5
MRX_ERR_INVALID = -1


def _sos(*parts):
    """A cascade from ("low" | "high", order) Bessel edges (order + 1 sections each, as
    process_tod builds them) or ready sos arrays."""
    from maria_amd import tod_processing as tp

    fc = {"low": 10.0, "high": 0.1}
    out = [tp.bessel_sos(fc[p[0]], FS, p[1], p[0]) if isinstance(p, tuple) else p for p in parts]
    return np.ascontiguousarray(np.concatenate(out, axis=0), np.float64)


def _rows(D, T, seed):
    """Random walk + white noise + an offset + a ramp per row, float32."""
    rng = np.random.default_rng(seed)
    x = np.empty((D, T), np.float32)
    ramp = np.linspace(0.0, 1.0, T)
    for d in range(D):
        x[d] = (np.cumsum(rng.normal(size=T)) * 0.05 + rng.normal(size=T) + rng.uniform(-50, 50) + rng.uniform(-20, 20) * ramp)
    return x


def _buffer(D, T, ld, off, x=None):
    """A flat device buffer of sentinels with a [D, ld] view starting `off` floats in; the first
    T columns hold x if given."""
    import torch

    flat = torch.full((off + D * ld + 5,), SENTINEL, dtype=torch.float32, device="cuda:0")
    view = flat[off : off + D * ld].view(D, ld)
    if x is not None:
        view[:, :T] = torch.as_tensor(x).to("cuda:0")
    return flat, view


def _untouched(flat, D, T, ld, off):
    """Everything of the flat buffer outside the [D, T] window is still the sentinel."""
    h = flat.cpu().numpy()
    mask = np.ones(h.size, bool)
    body = mask[off : off + D * ld].reshape(D, ld)
    body[:, :T] = False
    return bool((h[mask] == SENTINEL).all())


def _work(ctx, D, T, S):
    import torch

    need = C.c_size_t()
    assert ctx.lib.mrx_sosfilt_work_doubles(D, T, S, C.byref(need)) == 0
    return torch.empty(need.value, dtype=torch.float64, device="cuda:0")


def _chunk_matrix(ctx, sos):
    import torch

    from maria_amd import tod_processing as tp

    return torch.as_tensor(tp.chunk_matrix(sos, ctx.lib.mrx_sosfilt_chunk())).to("cuda:0")


def _sosfilt_rc(ctx, sos, n_sections, M, d_in, ld_in, D, T, remove_slope, d_out, ld_out, work):
    from maria_amd._lib import ptr

    return ctx.lib.mrx_sosfilt(ctx.handle, sos.ctypes.data_as(C.POINTER(C.c_double)), n_sections, ptr(M), ptr(d_in), ld_in, D, T,
                               remove_slope, ptr(d_out), ld_out, ptr(work))


def _ref_sosfilt(sos, x, remove_slope):
    x64 = x.astype(np.float64)
    if remove_slope:
        x64 = x64 - np.linspace(x64[:, 0], x64[:, -1], x.shape[1]).T
    return scipy.signal.sosfilt(sos, x64, axis=-1)


def _worst_row(got, ref, bound=3e-7):
    """Per row: max|got - ref| <= bound * max|ref_row|.  Returns the worst ratio err / max|ref_row|."""
    err = np.abs(got.astype(np.float64) - ref).max(axis=1)
    scale = np.abs(ref).max(axis=1)
    bad = np.flatnonzero(err > bound * scale)
    assert bad.size == 0, f"rows {bad[:8]}: err {err[bad[:8]]} vs bound {bound * scale[bad[:8]]}"
    return float((err / np.where(scale > 0, scale, 1.0)).max())


def _run_sosfilt(ctx, sos, x, remove_slope, layout):
    """mrx_sosfilt of x [D, T] in one of the layouts:
      inplace  ld = T + 3, the result over the input
      out      out of place, ld_in = round4(T) + 4 != ld_out = round4(T) + 8 (16-byte path)
      off1     out of place, both base pointers 1 float into their buffers (scalar path)
      off4     out of place, both base pointers 4 floats in, ld a multiple of 4 (16-byte path)
    checks the padding and, out of place, the input; returns the result [D, T]."""
    D, T = x.shape
    r4 = -(-T // 4) * 4
    ld_in, ld_out, off = {"inplace": (T + 3, T + 3, 0), "out": (r4 + 4, r4 + 8, 0), "off1": (T + 1, T + 5, 1),
                          "off4": (r4 + 4, r4 + 12, 4)}[layout]
    fin, vin = _buffer(D, T, ld_in, off, x)
    fout, vout = (fin, vin) if layout == "inplace" else _buffer(D, T, ld_out, off)
    M, work = _chunk_matrix(ctx, sos), _work(ctx, D, T, len(sos))
    assert _sosfilt_rc(ctx, sos, len(sos), M, vin, ld_in, D, T, remove_slope, vout, ld_out, work) == 0
    got = vout[:, :T].cpu().numpy()
    assert _untouched(fout, D, T, ld_out, off), "mrx_sosfilt wrote outside [D, T]"
    if layout != "inplace":
        assert _untouched(fin, D, T, ld_in, off) and np.array_equal(vin[:, :T].cpu().numpy(), x), "the input changed"
    return got


# every cascade length S = 1..8: low alone, high alone, both where S <= 8, two non-Bessel ones
CASCADES = ([("low", o) for o in range(8)] + [("high", o) for o in range(8)]
            + [(("low", a), ("high", b)) for a, b in [(0, 0), (1, 1), (2, 2), (3, 3), (0, 6), (6, 0), (2, 4)]]
            + ["butter", "cheby1"])


def _cascade(c):
    if c == "butter":
        return _sos(scipy.signal.butter(4, [0.2 / FS * 2, 20.0 / FS * 2], btype="band", output="sos"))
    if c == "cheby1":
        return _sos(scipy.signal.cheby1(5, 1.0, 30.0 / FS * 2, output="sos"))
    return _sos(*c) if isinstance(c[0], tuple) else _sos(c)


@pytest.mark.parametrize("cascade", CASCADES, ids=lambda c: str(c).replace(" ", ""))
def test_sosfilt_every_cascade(gpu_ctx, cascade):
    """Every instance launch_sos<S> has, at the existing test's T = 5000 with a partial last chunk."""
    sos = _cascade(cascade)
    x = _rows(9, 5000, seed=len(sos))
    w = max(_worst_row(_run_sosfilt(gpu_ctx, sos, x, remove_slope, "out"), _ref_sosfilt(sos, x, remove_slope)) for remove_slope in (0, 1))
    print(f"[todproc] sosfilt {cascade} S={len(sos)}: worst row err {w:.2e} max|ref_row|")


# (cascade, T, D, layout, remove_slope): every S, T and D of the chunk kernel's workgroups
# (65 536 samples) and the scan kernel's blocks (256 detectors) at least once
SHAPES = [
    (("low", 0), 65_535, 257, "inplace", 1),
    (("high", 1), 65_536, 256, "out", 0),
    (("low", 2), 65_537, 255, "off1", 1),
    ((("low", 1), ("high", 1)), 131_329, 1, "off4", 1),
    (("high", 4), 240_000, 1, "off1", 0),
    ((("low", 2), ("high", 2)), 5_000, 513, "off4", 1),
    (("low", 6), 131_329, 3, "inplace", 1),
    ((("low", 3), ("high", 3)), 240_000, 2, "off4", 1),
    ((("low", 3), ("high", 3)), 65_537, 257, "inplace", 1),
    ("butter", 65_536, 513, "out", 1),
    ("cheby1", 240_000, 5, "off1", 1),
]


@pytest.mark.parametrize("cascade,T,D,layout,remove_slope", SHAPES,
                         ids=[f"S{len(_cascade(s[0]))}-T{s[1]}-D{s[2]}-{s[3]}" for s in SHAPES])
def test_sosfilt_workgroups_and_layouts(gpu_ctx, cascade, T, D, layout, remove_slope):
    """Rows longer than one chunk workgroup (blockIdx.x > 0, a partial last workgroup and chunk)
    and more detectors than one scan block, in place, out of place and off the 16-byte path."""
    sos = _cascade(cascade)
    x = _rows(D, T, seed=T + D)
    got = _run_sosfilt(gpu_ctx, sos, x, remove_slope, layout)
    w = _worst_row(got, _ref_sosfilt(sos, x, remove_slope))
    print(f"[todproc] sosfilt S={len(sos)} T={T} D={D} {layout}: worst row err {w:.2e} max|ref_row|")


def test_sosfilt_near_unit_poles(gpu_ctx):
    """High pass at f / fs = 1e-5 (0.004 Hz at 400 Hz, order 3) over 240 000 samples: the poles
    sit next to 1, and the chained chunk states carry almost all of the signal."""
    from maria_amd import tod_processing as tp

    sos = _sos(tp.bessel_sos(0.004, FS, 3, "high"))
    x = _rows(4, 240_000, seed=11)
    got = _run_sosfilt(gpu_ctx, sos, x, 1, "out")
    w = _worst_row(got, _ref_sosfilt(sos, x, 1))
    print(f"[todproc] sosfilt near-unit poles: worst row err {w:.2e} max|ref_row|")


@pytest.mark.parametrize("n_sections,D", [(0, 4), (9, 4), (4, 65_536)])
def test_sosfilt_refusals(gpu_ctx, n_sections, D):
    """0 or 9 sections, and more rows than one launch's grid.y: MRX_ERR_INVALID, nothing written."""
    import torch

    T = 8
    sos = _sos(("low", 1), ("high", 1), ("low", 3))  # 8 sections; the refused calls read at most n_sections
    sos9 = _sos(("low", 3), ("high", 4))
    src = sos9 if n_sections == 9 else sos
    x = torch.ones(D, T, dtype=torch.float32, device="cuda:0")
    out = torch.full((D, T), SENTINEL, dtype=torch.float32, device="cuda:0")
    M = torch.zeros(18, 18, dtype=torch.float64, device="cuda:0")
    work = torch.zeros(2 * D + D * 18 + 16, dtype=torch.float64, device="cuda:0")
    rc = _sosfilt_rc(gpu_ctx, src, n_sections, M, x, T, D, T, 1, out, T, work)
    torch.cuda.synchronize()
    assert rc == MRX_ERR_INVALID, rc
    assert bool((out == SENTINEL).all()) and bool((x == 1).all()) and bool((work == 0).all())
    need = C.c_size_t()
    if n_sections in (0, 9):
        assert gpu_ctx.lib.mrx_sosfilt_work_doubles(D, T, n_sections, C.byref(need)) == MRX_ERR_INVALID


def test_sosfilt_and_detrend_full_size_sampled_rows(gpu_ctx):
    """process_tod's cascade for {"f_lower": 0.1, "f_upper": 10.0} at 400 Hz on 10 000 x 240 000
    (the mapper benchmarks' TOD), remove_slope, out of place; ~40 rows against scipy, a second
    call bit-identical; then mrx_tod_detrend_window (slope + hann) at the same size."""
    import torch

    from maria_amd._lib import ptr

    D, T = 10_000, 240_000
    gen = torch.Generator(device="cuda:0").manual_seed(20261015)
    x = torch.empty(D, T, dtype=torch.float32, device="cuda:0")
    ramp = torch.linspace(0.0, 1.0, T, dtype=torch.float32, device="cuda:0")
    for lo in range(0, D, 1000):
        blk = x[lo : lo + 1000]
        torch.randn(blk.shape, generator=gen, device="cuda:0", out=blk)
        blk.cumsum_(dim=1)
        blk.mul_(0.05).add_(torch.randn(blk.shape, generator=gen, device="cuda:0"))
        blk.add_(torch.rand(1000, 1, generator=gen, device="cuda:0") * 100 - 50)
        blk.add_((torch.rand(1000, 1, generator=gen, device="cuda:0") * 40 - 20) * ramp)
    rng = np.random.default_rng(5)
    rows = np.unique(np.r_[0, 255, 256, 257, D - 1, rng.choice(D, 35, replace=False)])
    idx = torch.as_tensor(rows, device="cuda:0")
    xs = x[idx].cpu().numpy()

    sos = _sos(("low", 1), ("high", 1))
    M, work = _chunk_matrix(gpu_ctx, sos), _work(gpu_ctx, D, T, len(sos))
    out = torch.empty_like(x)
    assert _sosfilt_rc(gpu_ctx, sos, len(sos), M, x, T, D, T, 1, out, T, work) == 0
    w = _worst_row(out[idx].cpu().numpy(), _ref_sosfilt(sos, xs, 1))
    again = torch.empty_like(x)
    assert _sosfilt_rc(gpu_ctx, sos, len(sos), M, x, T, D, T, 1, again, T, work) == 0
    assert torch.equal(out, again)
    del out, again, work
    assert torch.equal(x[idx].cpu(), torch.as_tensor(xs))

    win = scipy.signal.windows.hann(T)
    d_w = torch.as_tensor(win).to("cuda:0")
    anchors = torch.empty(2 * D, dtype=torch.float64, device="cuda:0")
    gpu_ctx.call("mrx_tod_detrend_window", ptr(x), T, D, T, 1, ptr(d_w), ptr(anchors))
    got = x[idx].cpu().numpy()
    del x, d_w, anchors
    torch.cuda.empty_cache()
    ref = xs.copy()
    ref -= np.linspace(ref[:, 0], ref[:, -1], T).T
    ref *= win
    frac = _ulp_check(got, ref)
    print(f"[todproc] full size sosfilt: worst row err {w:.2e} max|ref_row|; detrend bit-equal {frac:.6f}")


def _ulp_check(got, ref):
    """Every sample within 1 float32 ulp of numpy's, 99.99 % bit-equal; returns the bit-equal fraction."""
    assert got.dtype == ref.dtype == np.float32
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(ref))).astype(np.float64)
    assert (diff <= ulp).all(), f"{int((diff > ulp).sum())} samples beyond 1 ulp; worst {(diff / ulp).max():.1f} ulp"
    frac = float((got == ref).mean()) if got.size else 1.0
    assert frac >= 0.9999, frac
    return frac


DETREND_FLAGS = {"slope": (1, None), "tukey": (0, ("tukey", {"alpha": 0.2})), "hann": (0, ("hann", {})),
                 "slope+tukey": (1, ("tukey", {"alpha": 0.5})), "slope+hann": (1, ("hann", {}))}


@pytest.mark.parametrize("flags", list(DETREND_FLAGS))
def test_detrend_window_matches_numpy_in_place(gpu_ctx, flags):
    """D -= np.linspace(D[:, 0], D[:, -1], T).T; D *= w on float32, as process_tod's reference does
    (numpy evaluates the line in float32): D not a multiple of the kernel's 16-row block, T = 1, 2,
    3 and around its 256-sample block, ld > T with sentinels in the padding."""
    import torch

    from maria_amd._lib import ptr

    slope, window = DETREND_FLAGS[flags]
    equal = total = 0
    for D in (1, 15, 16, 17, 1000):
        for T in (1, 2, 3, 255, 257, 4099):
            x = _rows(D, T, seed=D * 10_000 + T)
            ld = T + 3
            flat, view = _buffer(D, T, ld, 0, x)
            w = getattr(scipy.signal.windows, window[0])(T, **window[1]) if window else None
            d_w = torch.as_tensor(w).to("cuda:0") if window else None
            anchors = torch.empty(2 * D, dtype=torch.float64, device="cuda:0")
            gpu_ctx.call("mrx_tod_detrend_window", ptr(view), ld, D, T, slope, ptr(d_w) if window else None, ptr(anchors))
            got = view[:, :T].cpu().numpy()
            assert _untouched(flat, D, T, ld, 0), (D, T)
            ref = x.copy()
            if slope:
                ref -= np.linspace(ref[:, 0], ref[:, -1], T).T
            if window:
                ref *= w
            _ulp_check(got, ref)
            equal += int((got == ref).sum())
            total += got.size
    print(f"[todproc] detrend {flags}: bit-equal {equal / total:.6f} of {total}")


def test_detrend_window_neither_flag_is_a_no_op(gpu_ctx):
    """Neither remove_slope nor a window: the buffer is left alone and no scratch is needed."""
    x = _rows(17, 257, seed=1)
    flat, view = _buffer(17, 257, 260, 0, x)
    before = flat.clone()
    from maria_amd._lib import ptr

    gpu_ctx.call("mrx_tod_detrend_window", ptr(view), 260, 17, 257, 0, None, None)
    import torch

    torch.cuda.synchronize()
    assert torch.equal(flat, before)
