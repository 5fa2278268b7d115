"""The K_RJ division's per-tile model, form by form, against float64: mrx_tod_to_krj, mrx_tod_from_krj and
mrx_coarse_to_krj on every case of tests/krj_ref.py -- the device's own detector elevation through ramp tables (den = el),
the cell, the kink and the NaNs through zigzag tables on which a neighbouring cell costs 2e-2 -- every sample held to an
allowance that comes from the reference alone (tests/test_host_krj_ref.py); and the writers that inline the same header
(the noise writer, the spline writer) against the pW field converted afterwards on the tracks that leave the usual form.

Every test prints its largest error per form beside its allowance ("krj: ..."), the figures DESIGN 3.7 quotes."""

import ctypes as C
import functools

import krj_ref as kr
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = kr.cases()
case_param = pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
EL_ROUND = 1.6 * kr.ULP  # rad: the float32 rounding of an elevation below 1.6 rad on its way out (1 x den)


def _t(a, dtype=np.float32):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _pointing(case):
    return dict(bore=_t(case.bore_el), dx=_t(case.off[:, 0]), dy=_t(case.off[:, 1]), band=_t(case.band, np.int32))


@functools.lru_cache(maxsize=None)
def _table(case, kind):
    axis, values = case.table(kind)
    return _t(axis), _t(values), len(axis), values.shape[0]


def _cal(case, kind):
    """bore_el, dx, dy, band, axis, values, n_el, n_bands: the tail of every K_RJ entry"""
    from maria_amd._lib import ptr

    p, (axis, values, n_el, nb) = _pointing(case), _table(case, kind)
    return ptr(p["bore"]), ptr(p["dx"]), ptr(p["dy"]), ptr(p["band"]), ptr(axis), ptr(values), n_el, nb


def _convert(ctx, entry, case, kind, x):
    """mrx_tod_to_krj / mrx_tod_from_krj of x [D, T] in place in rows of ceil4(T) + pad floats (pad = 0: 16-byte loads and
    stores; pad = 3: the scalar path): [D, T] float64 on the host; the floats behind every row untouched."""
    import torch

    from maria_amd._lib import ptr

    D, T = case.shape
    ld = (T + 3) // 4 * 4 + case.pad
    buf = torch.full((D, ld), 7.0, dtype=torch.float32, device=DEV)
    buf[:, :T] = _t(x)
    assert (buf.data_ptr() % 16 == 0) and (ld % 4 == 0) == (case.pad == 0)
    ctx.call(entry, ptr(buf), ld, D, T, None, None, *_cal(case, kind))
    out = buf.cpu().numpy()
    assert (out[:, T:] == 7.0).all()
    return out[:, :T].astype(np.float64)


def _report(what, case, kind, err, allow, ok):
    """One line: per form of the restatement the largest error beside the largest allowance; the assertion's message."""
    form = case.form_of_samples(kind, kr.CURVATURE_GATE)
    over = case.straddling(kind)  # the threads whose four samples have a node between them: a class of their own
    parts = []
    for code, name in enumerate(kr.FORMS + ("straddling",)):
        m = (over if name == "straddling" else (form == code) & ~over) & np.isfinite(err)
        if m.any():
            parts.append(f"{name} {err[m].max():.2e} / {allow[m].max():.2e}")
    print(f"\nkrj: {what} {case.name} {kind}: B_el {case.b_el.max():.2e} (chain {case.delta_chain:.2e}); error / allowance: " + "; ".join(parts))
    if ok.all():
        return ""
    d, s = np.argwhere(~ok)[0]
    return (f"{int((~ok).sum())} of {ok.size} samples beyond their allowance; first: row {d} sample {s} ({kr.FORMS[form[d, s]]}): "
            f"{err[d, s]:.3e} > {allow[d, s]:.3e}; worst {np.nanmax(err / allow):.2f} x the allowance")


def _held(got, ref, allow, exempt):
    """(error, ok): |got / ref - 1| within the allowance on every sample of the reference, NaN where the reference has
    them and nowhere else -- but for the samples within B_el of an end of the axis, which may go either way."""
    err = np.abs(got / ref - 1.0)
    nan_ok = (np.isnan(got) == np.isnan(ref)) | exempt
    ok = nan_ok & (np.isnan(ref) | np.isnan(got) | (err <= allow))
    return err, ok


@pytest.mark.parametrize("kind", ["ramp3", "ramp200"])
@case_param
def test_elevation_through_a_ramp_table(gpu_ctx, case, kind):
    """den = el on every node: mrx_tod_from_krj of ones is the device's own detector elevation, mrx_tod_to_krj its
    reciprocal.  |device - el_exact| <= B_el + 1.6 x 2^-24 on every sample (B_el = 1e-6 rad + the float32 chain's own
    distance from el_exact + the inner samples' deviation from the chord); three nodes: nearly every row linear; 200
    nodes (0.35 deg cells): rows sweep more than two cells a tile and go sample by sample on the linear model."""
    ref, exempt = case.den(kind), case.exempt(kind)
    ones = np.ones(case.shape, np.float32)
    got = _convert(gpu_ctx, "mrx_tod_from_krj", case, kind, ones)
    err = np.abs(got - ref)
    allow = np.broadcast_to(case.b_el + EL_ROUND, err.shape)
    ok = ((np.isnan(got) == np.isnan(ref)) | exempt) & (np.isnan(ref) | np.isnan(got) | (err <= allow))
    msg = _report("el (from_krj)", case, kind, err, allow, ok)
    assert ok.all(), msg
    inv = _convert(gpu_ctx, "mrx_tod_to_krj", case, kind, ones)
    err, ok = _held(inv, 1.0 / ref, case.tol(kind), exempt)
    msg = _report("1 / el (to_krj)", case, kind, err, case.tol(kind), ok)
    assert ok.all(), msg


@case_param
def test_coarse_form_takes_the_chain_itself(gpu_ctx, case):
    """mrx_coarse_to_krj with the track as the coarse boresight, a loading of ones, the 200-node ramp: 1 / el with
    asinf per step -- no model, no Newton step: the float32 chain's own distance from el_exact plus rounding."""
    import torch

    from maria_amd._lib import ptr

    D, T = case.shape
    kind = "ramp200"
    loading = torch.ones((T, D), dtype=torch.float32, device=DEV)
    out = torch.full((T, D), 7.0, dtype=torch.float32, device=DEV)
    gpu_ctx.call("mrx_coarse_to_krj", ptr(loading), D, T, *_cal(case, kind), ptr(out))
    got = out.cpu().numpy().T.astype(np.float64)
    ref = case.den(kind)
    b = case.delta_chain + EL_ROUND
    allow = np.broadcast_to(b / np.abs(case.el) + 3 * kr.ULP, ref.shape)
    err, ok = _held(got, 1.0 / ref, allow, kr.near_an_end(case.table(kind)[0], case.el, b))
    print(f"\nkrj: coarse {case.name}: chain {case.delta_chain:.2e}; largest error {np.nanmax(err):.2e} / allowance {allow[np.isfinite(err)].max():.2e}")
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:3], float(np.nanmax(err / allow)))


@pytest.mark.parametrize("kind", ["zigzag", "nonuniform"])
@case_param
def test_cells_kinks_and_nans(gpu_ctx, case, kind):
    """Both directions on the zigzag tables: |got / ref - 1| <= tol on every sample, the NaNs where the reference has
    them, and from_krj(to_krj(x)) within 4 x 2^-24 of x (relative: a reciprocal to an ulp and three roundings)."""
    rng = np.random.default_rng(11)
    x = rng.uniform(1.0, 2.0, case.shape).astype(np.float32)
    den, tol, exempt = case.den(kind), case.tol(kind), case.exempt(kind)
    to = _convert(gpu_ctx, "mrx_tod_to_krj", case, kind, x)
    err, ok = _held(to, x / den, tol, exempt)
    msg = _report("to_krj", case, kind, err, tol, ok)
    assert ok.all(), msg
    frm = _convert(gpu_ctx, "mrx_tod_from_krj", case, kind, x)
    err, ok = _held(frm, x * den, tol, exempt)
    msg = _report("from_krj", case, kind, err, tol, ok)
    assert ok.all(), msg
    back = _convert(gpu_ctx, "mrx_tod_from_krj", case, kind, to.astype(np.float32))
    trip = np.abs(back / x - 1.0)
    print(f"krj: round trip {case.name} {kind}: {np.nanmax(trip) / kr.ULP:.2f} x 2^-24")
    assert np.array_equal(np.isnan(back), np.isnan(to)) and not (trip > 4 * kr.ULP).any()


def test_every_tile_decides_for_itself(gpu_ctx):
    """One track whose first tile is linear, whose second is a slew past the model's range (every row exact) and whose
    third leaves the axis: the range reduction (red[]) is the workgroup's own."""
    case, kind = kr.case("tiles"), "zigzag"
    f = case.forms(kind, kr.CURVATURE_GATE)
    assert np.isin(f[0], (kr.LIN, kr.KINK)).all() and (f[1] == kr.EXACT).all() and (f[2] == kr.SAMPLE).any()
    den = case.den(kind)
    assert np.isfinite(den[:, : 2 * kr.TILE]).all() and np.isnan(den[:, 2 * kr.TILE :]).any() and np.isfinite(den[:, 2 * kr.TILE :]).any()
    got = _convert(gpu_ctx, "mrx_tod_to_krj", case, kind, np.ones(case.shape, np.float32))
    err, ok = _held(got, 1.0 / den, case.tol(kind), case.exempt(kind))
    for k in range(len(f) - 1):  # (the fourth tile: five samples, every one off the axis)
        s = slice(k * kr.TILE, (k + 1) * kr.TILE)
        print(f"krj: tile {k}: forms {sorted({kr.FORMS[c] for c in f[k]})}, largest error {np.nanmax(err[:, s]):.2e} / allowance {np.nanmax(case.tol(kind)[:, s]):.2e}")
    assert ok.all(), np.argwhere(~ok)[:3]


# ---- the writers that inline the same division ----

TRACKS = ("sweep_60_under", "sweep_68_over", "steep", "curved", "off_low", "off_high")
AXES = {"off_low": (60.0, 90.0), "off_high": (20.0, 62.0)}


@functools.lru_cache(maxsize=None)
def _writer_case(track, T):
    off = kr.case("sweep_60_under" if track.startswith("sweep") else "lin").off
    return kr._case(f"{track}_{T}", [], off, kr.track(track, T), axis_deg=AXES.get(track, (20.0, 90.0)))


def _same(got, ref, rel=0.0):
    """NaN for NaN, and elsewhere the same bits (rel = 0) or within rel of the reference."""
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    if rel == 0.0:
        return np.array_equal(got[~nan], ref[~nan]), float(nan.mean())
    return bool((np.abs(got[~nan].astype(np.float64) / ref[~nan] - 1.0) <= rel).all()), float(nan.mean())


@pytest.mark.parametrize("T,fs,knee", [(9000, 100.0, 1.0), (33001, 400.0, 1.0)], ids=["one_rate", "two_rate"])
@pytest.mark.parametrize("track", TRACKS)
def test_noise_written_in_krj_on_every_form(gpu_ctx, track, T, fs, knee):
    """mrx_noise_generate_krj against mrx_noise_generate then mrx_tod_to_krj, bit for bit and NaN for NaN, on the tracks
    that leave the usual form.  T = 9000: the one-rate form (the call is the two in turn); T = 33001 at 400 Hz: the
    two-rate writer's own store, the division inlined in mrx_noise.hip."""
    import torch

    from maria_amd import _lib
    from maria_amd._lib import ptr

    case = _writer_case(track, T)
    D = case.shape[0]
    rng = np.random.default_rng(5)
    n_modes = 3
    basis, scale = _t(rng.normal(size=(D, n_modes))), _t(rng.uniform(1.0, 2.0, D))
    need = C.c_size_t()
    _lib.load().mrx_noise_work_floats(T, n_modes, D, C.byref(need))
    work = torch.empty(need.value, dtype=torch.float32, device=DEV)
    head = (77, D, 0, T, fs, knee, 0.5, ptr(basis), n_modes, ptr(scale), None, 0, 0.0)
    plain = torch.empty((D, T), dtype=torch.float32, device=DEV)
    gpu_ctx.call("mrx_noise_generate", *head, ptr(plain), plain.stride(0), 0, ptr(work), need.value)
    fused = torch.empty((D, T), dtype=torch.float32, device=DEV)
    gpu_ctx.call("mrx_noise_generate_krj", *head, ptr(fused), fused.stride(0), ptr(work), need.value, *_cal(case, "zigzag"))
    gpu_ctx.call("mrx_tod_to_krj", ptr(plain), plain.stride(0), D, T, None, None, *_cal(case, "zigzag"))
    torch.cuda.synchronize()
    same, nans = _same(fused, plain)
    forms = sorted({kr.FORMS[c] for c in case.forms("zigzag", kr.CURVATURE_GATE).ravel()})
    print(f"\nkrj: noise writer {track} T {T}: forms {forms}, NaN share {nans:.3f}, bit for bit {same}")
    assert same and (nans > 0) == track.startswith("off")


@pytest.mark.parametrize("track", TRACKS)
def test_spline_written_in_krj_on_every_form(gpu_ctx, track):
    """mrx_spline_upsample_krj against mrx_spline_upsample then mrx_tod_to_krj: the same lookup, one more float32
    rounding (the pW value is stored before the division): 3e-7, NaN for NaN."""
    import torch

    from maria_amd._lib import ptr

    T, per_knot = 9000, 50
    case = _writer_case(track, T)
    D = case.shape[0]
    Ta = T // per_knot + 2
    rng = np.random.default_rng(6)
    loading = _t(1.5 + 0.01 * np.cumsum(rng.normal(size=(Ta, D)), axis=0))
    ym = torch.empty((Ta, D, 2), dtype=torch.float32, device=DEV)
    gpu_ctx.call("mrx_spline_prepare", ptr(loading), D, Ta, ptr(ym))
    t = _t(np.arange(T) / 100.0, np.float64)
    grid = (ptr(ym), D, Ta, 0.0, per_knot / 100.0, ptr(t), T, None, None)
    plain = torch.empty((D, T), dtype=torch.float32, device=DEV)
    gpu_ctx.call("mrx_spline_upsample", *grid, ptr(plain), plain.stride(0))
    fused = torch.empty((D, T), dtype=torch.float32, device=DEV)
    gpu_ctx.call("mrx_spline_upsample_krj", *grid, *_cal(case, "zigzag"), ptr(fused), fused.stride(0))
    gpu_ctx.call("mrx_tod_to_krj", ptr(plain), plain.stride(0), D, T, None, None, *_cal(case, "zigzag"))
    torch.cuda.synchronize()
    same, nans = _same(fused, plain, rel=3e-7)
    print(f"\nkrj: spline writer {track}: NaN share {nans:.3f}, within 3e-7 {same}")
    assert same and (nans > 0) == track.startswith("off")
