"""Host geometry of the atmosphere -> TOD path: what ``DevicePath`` (pipeline.py) works out in numpy before it
launches anything -- the tables it uploads, the detector order, and the estimates that decide which kernel form a
run takes.  Plain functions of the problem and the calibration arrays; no torch, no device."""

from __future__ import annotations

import numpy as np


def matern_log_tables(nu, n=8192, lo=1e-6, hi=1e3, eps=1e-10):
    """log of the exact Matern correlation (functions/__init__.py:30-39) and of its complement at ``n``
    log-spaced r / r0 -- the construction of the reference's ``approximate_normalized_matern`` (:42-74), eight
    times denser because the device interpolates it to 1e-11 (``mrx_screen_amplitudes``).  Returns
    (log_first, log_step, log_cov, log_sf, x_cut); values the float64 range cannot hold (rho underflows
    beyond r ~ 700 r0) are pinned at log(1e-300); ``x_cut``: the first node where the correlation has fallen
    below ``eps`` (periodic images farther away are not summed)."""
    import scipy.special

    x = np.geomspace(lo, hi, n)
    z = np.sqrt(2 * nu) * x + 1e-16
    cov = 2 ** (1 - nu) / scipy.special.gamma(nu) * scipy.special.kv(nu, z) * z**nu
    with np.errstate(divide="ignore"):
        log_cov = np.maximum(np.log(cov), np.log(1e-300))
        log_sf = np.maximum(np.log(1 - cov), np.log(1e-300))
    lx = np.log(x)
    x_cut = float(x[np.argmax(cov < eps)]) if (cov < eps).any() else float(hi)
    return float(lx[0]), float((lx[-1] - lx[0]) / (n - 1)), np.ascontiguousarray(log_cov), np.ascontiguousarray(log_sf), x_cut


def morton_order(offsets):
    """Permutation that sorts focal-plane offsets along a Z-order curve, so that
    consecutive detectors (the lanes of a wave, the 256 rows of a workgroup) form a
    compact patch on the sky: their lines of sight then hit the same few cache lines
    of every screen.  Pure host-side indexing; results do not depend on it."""
    off = np.asarray(offsets, float)
    if len(off) < 2:
        return np.arange(len(off))
    off = np.where(np.isfinite(off), off, 0.0)  # (a NaN offset sorts anywhere; its samples are NaN whatever its place)
    lo, span = off.min(axis=0), np.maximum(np.ptp(off, axis=0), 1e-300)
    q = np.minimum(((off - lo) / span * 65535.0).astype(np.uint64), 65535)

    def spread(v):  # 16 bits -> every other bit of 32
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555

    return np.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1), kind="stable")


def f32_cell(axis, x):
    """The cell of ``axis`` that holds the scalar ``x``, exactly as jax's ``_find_indices`` finds it in float32
    (band/band.py:283-286): (index of the cell's lower node, clamped onto the axis; x's float32 normalised distance
    from that node; whether x lies off the axis)."""
    g = np.asarray(axis, np.float32)
    x = np.float32(x)
    i = int(np.searchsorted(g, x, side="left")) - 1
    i = min(max(i, 0), len(g) - 2)
    w = np.float32((x - g[i]) / (g[i + 1] - g[i]))
    return i, w, bool(x < g[0] or x > g[-1])


def table_slabs(table, T0):
    """Host part of the emission lookup: the two temperature slabs bracketing
    ``T0`` and T0's float32 normalised distance, computed exactly as jax's
    ``_find_indices`` would (f32_cell)."""
    i, w, oob = f32_cell(table["T"], T0)
    vals = np.asarray(table["values"], np.float32)[i : i + 2]
    return np.ascontiguousarray(vals), w, oob


def table_cubic_cells(table, T0):
    """Host part of ``interpolation_method="cubic"`` (band/band.py:288-300): the band table
    interpolated linearly to ``T0`` (scipy ``interp1d``, which raises ValueError outside the
    temperature axis, as in the reference) and scipy's tensor-product not-a-knot cubic spline on
    (pwv, el) expanded into one bicubic per grid cell (Taylor coefficients at the cell's lower
    corner).  Returns the float64 buffer of ``mrx_band_table.d_cubic``:
    [pwv nodes][el nodes][cells][16]."""
    import scipy.interpolate

    Tg, x, y = (np.asarray(table[k], float) for k in ("T", "pwv", "el"))
    V = scipy.interpolate.interp1d(Tg, np.asarray(table["values"], float), kind="linear", axis=0)(T0)  # [n_pwv, n_el]
    if len(x) < 4 or len(y) < 4:
        raise ValueError("cubic interpolation needs at least 4 nodes per axis")
    fact = (1.0, 1.0, 2.0, 6.0)
    # The reference calls scipy's RegularGridInterpolator(method="cubic").  From scipy 1.13 on that
    # is an NdBSpline whose coefficients come from an ITERATIVE solver (gcrotmk, atol 1e-6): it
    # differs from the exact tensor-product spline by ~6e-6 of the table's scale.  To reproduce the
    # reference and not the textbook, the cells are expanded from scipy's own spline object; older
    # scipy (recursive 1-D splines, exact) and the fallback below give the exact tensor spline.
    spline = getattr(scipy.interpolate.RegularGridInterpolator((x, y), V, method="cubic"), "_spline", None)
    if spline is not None and hasattr(spline, "t"):
        X0, Y0 = np.meshgrid(x[:-1], y[:-1], indexing="ij")
        pts = np.stack([X0.ravel(), Y0.ravel()], axis=-1)
        Cc = np.empty((len(x) - 1, len(y) - 1, 4, 4))
        for k in range(4):
            for m in range(4):
                Cc[:, :, k, m] = spline(pts, nu=(m, k)).reshape(len(x) - 1, len(y) - 1) / (fact[m] * fact[k])
    else:  # separable operator: Taylor coefficients in el of every pwv row's spline, then along pwv
        sy = scipy.interpolate.make_interp_spline(y, V, k=3, axis=1)
        A = np.stack([sy.derivative(k)(y[:-1]) / fact[k] if k else sy(y[:-1]) for k in range(4)], axis=-1)  # [n_pwv, n_el-1, 4]
        sx = scipy.interpolate.make_interp_spline(x, A, k=3, axis=0)
        Cc = np.stack([sx.derivative(m)(x[:-1]) / fact[m] if m else sx(x[:-1]) for m in range(4)], axis=-1)  # [.., 4(k), 4(m)]
    return np.concatenate([x, y, np.ascontiguousarray(Cc).reshape(-1)])


def layer_offsets(timestep, layer):
    """f64 per-time offsets of mrx_layer (include/mrx.h):
    (cumsum(timestep*(vx,vy,0)) + (0,0,h)) @ transform, columns 0 and 1
    (atmosphere/atmosphere.py:318-319,346-347)."""
    tr = np.cumsum(timestep * np.c_[layer["vx"], layer["vy"], np.zeros(len(layer["vx"]))], axis=0)
    q = (tr + np.array([0.0, 0.0, layer["h"]])) @ np.asarray(layer["transform"], float)
    return q[:, 0], q[:, 1]


def sampled_margins_px(problem):
    """Per layer, the smallest distance in pixels between any line of sight of the observation and an edge of the
    layer's grid: (margin along the extrusion axis, margin across).  Of the WHOLE focal plane, not of one path's
    detector shard: the margins decide how a screen is generated (the beam as a stencil or as a factor of the
    spectrum, generate_screens), screens are shared by all shards -- regenerated by every rank or, layer-sharded,
    made by one rank for all --, and a shard's TOD must not depend on how the detectors were cut.  Host-side and
    conservative: the boresight track with a ring of 24 directions around the focal plane's outermost detector,
    pushed out to circumscribe the circle, through the float64 form of the pointing
    (coords/transforms.py:10-29) and the layer's projection (atmosphere/atmosphere.py:346-347)."""
    off = np.asarray(problem["offsets"], float)
    rad = float(np.hypot(off[:, 0], off[:, 1]).max()) if len(off) else 0.0
    ang = np.linspace(0.0, 2.0 * np.pi, 24, endpoint=False)
    ring = np.r_[np.zeros((1, 2)), (rad / np.cos(np.pi / 24) * 1.001 + 1e-9) * np.c_[np.cos(ang), np.sin(ang)]]
    az, el = np.asarray(problem["az_a"], float), np.asarray(problem["el_a"], float)
    dx, dy = ring[:, 0][:, None], ring[:, 1][:, None]
    r, q = np.hypot(dx, dy), np.arctan2(-dx, -dy)
    z = (np.sin(r) * np.cos(q) + 1j * np.cos(r)) * np.exp(1j * (el[None, :] - np.pi / 2))
    phi, theta = np.arctan2(np.sin(r) * np.sin(q), z.real) + az[None, :], np.arcsin(z.imag)
    with np.errstate(divide="ignore", invalid="ignore"):
        px, py = np.cos(phi) / np.tan(theta), np.sin(phi) / np.tan(theta)
    out = []
    for layer in problem["layers"]:
        oe, oc = layer_offsets(problem["timestep"], layer)
        R = np.asarray(layer["transform"], float)
        e = layer["h"] * (px * R[0, 0] + py * R[1, 0]) + oe[None, :]
        c = layer["h"] * (px * R[0, 1] + py * R[1, 1]) + oc[None, :]
        ex, cs = np.asarray(layer["extrusion"], float), np.asarray(layer["cross_section"], float)
        de, dc = (ex[-1] - ex[0]) / (len(ex) - 1), (cs[-1] - cs[0]) / (len(cs) - 1)
        if not (np.isfinite(e).all() and np.isfinite(c).all()):
            out.append((-np.inf, -np.inf))
            continue
        out.append((float(min(e.min() - ex[0], ex[-1] - e.max()) / de), float(min(c.min() - cs[0], cs[-1] - c.max()) / dc)))
    return out


def krj_split(t, ta, T):
    """Samples up to the last coarse knot.  Past it the reference EXTRAPOLATES its spline of the loading and divides
    by the true denominator; the coarse-grid form would extrapolate loading / denominator instead, and an extrapolated
    cubic misses the denominator's motion by 50x what an interior interval does (9e-5 in the last four samples of a
    tight fast scan, found by the randomised front-end sweep) -- so those samples, at most one coarse step of them,
    take the per-sample form: the two-call spline of the last knots and mrx_spline_upsample_krj on that window."""
    return int(np.searchsorted(np.asarray(t, float)[:T], float(ta[-1]), side="right"))


def collapse_calibration(cal_tables, base_temperature, zenith_pwv, polarized=None):
    """The K_RJ denominator on the elevation axis (tod/tod.py:90-142, calibration/functions.py:73-90,
    band/band.py:235-255): every band's (T, pwv, el) table of trapezoid(passband * exp(-opacity), nu) collapsed at the
    scalar (``base_temperature``, ``zenith_pwv``) with jax's float32 index/weight rule (f32_cell) and scaled to
    den = factor * k_B * 1e12 * integral, so that K_RJ = pW / den.  All bands share the elevation axis (one
    spectrum).  Returns (el_axis float64 [n_el], dens float32 [n_bands, n_el]; NaN where a scalar is off its axis)."""
    k_B = 1.380649e-23
    nb = len(cal_tables)
    el_axis = np.asarray(cal_tables[0]["el"], float)
    polarized = np.zeros(nb, bool) if polarized is None else np.asarray(polarized, bool)
    dens = np.zeros((nb, len(el_axis)), np.float32)
    for b, tab in enumerate(cal_tables):
        assert np.array_equal(np.asarray(tab["el"], float), el_axis), "bands must share the elevation axis"
        vals = np.asarray(tab["values"], np.float32).astype(np.float64)
        (it, wt, ot), (ip, wp, op) = f32_cell(tab["T"], base_temperature), f32_cell(tab["pwv"], zenith_pwv)
        wt, wp = float(wt), float(wp)
        sl = vals[it : it + 2, ip : ip + 2]  # [2, 2, nel]
        col = ((1 - wt) * (1 - wp)) * sl[0, 0] + ((1 - wt) * wp) * sl[0, 1] + (wt * (1 - wp)) * sl[1, 0] + (wt * wp) * sl[1, 1]
        if ot or op:
            col = np.full_like(col, np.nan)
        dens[b] = ((0.5 if polarized[b] else 1.0) * k_B * 1e12 * col).astype(np.float32)
    return el_axis, dens


# the coarse-grid form of the K_RJ conversion is taken when this estimate of its deviation from the
# per-sample form stays below 0.4 of the parity tolerance (1e-5): the float32 path itself takes 3e-6 of it
# at full size, which leaves a quarter of the tolerance unspent
COARSE_KRJ_LIMIT = 4.0e-6
SPLINE_KINK = 0.1708  # max |spline - f| / (slope jump x knot spacing) for a kink between uniform knots


def coarse_krj_bound(el_axis, dens, radius, el_a, t, ta):
    """Estimate of max |S[y/g] - S[y]/g| / |S[y]/g| (S: the spline in time, g: the K_RJ
    denominator at the detector's elevation), i.e. of what dividing the COARSE loading by g
    (mrx_coarse_to_krj, then the pW writer) changes against dividing every full-rate sample
    (mrx_spline_upsample_krj, the reference's order, tod/tod.py:106-142).  Both are the same
    linear functional of y but for the spline's interpolation error on g(t) = den(el(t)):
    (a) where a detector's elevation crosses a node of the table's axis between two knots g has
    a kink, and the not-a-knot cubic spline through uniform knots misses a kink by at most 0.1708 x
    (slope jump) x (knot spacing) -- the kink in the middle of a knot interval; 0.085 on a knot; a
    linear interpolant: 0.25 -- (tests/test_host_geometry.py::test_spline_error_at_a_kink computes it);
    measured on the daisy scan: 0.15;
    (b) inside a cell g is linear in el, so the error is the spline's error on el(t),
    (5/384) h^4 d4el/dt4 -- estimated from fourth differences of the coarse boresight.
    inf when the form does not apply: a NaN in the collapsed table, a detector that may leave
    the table's elevation axis, or one that comes within 7 deg of the zenith (its elevation
    is not smooth in time there).
    ``el_axis``, ``dens``: of collapse_calibration (taken as the device holds them, in float32); ``radius``: of the
    WHOLE focal plane; ``el_a``, ``ta``: the coarse boresight elevation and its times; ``t``: the sample times."""
    ax, den = np.asarray(el_axis, np.float32).astype(np.float64), np.asarray(dens, np.float32).astype(np.float64)
    el = np.asarray(el_a, float)
    if not np.isfinite(den).all() or len(el) < 5:
        return float("inf")
    lo, hi = el.min() - 1.05 * radius, el.max() + 1.05 * radius
    if lo < ax[0] or hi > ax[-1] or hi > np.radians(83.0):
        return float("inf")
    # only the part of the axis the detectors visit counts: the cells that overlap [lo, hi] and the
    # nodes between them
    i0 = max(int(np.searchsorted(ax, lo, side="right")) - 1, 0)
    i1 = min(int(np.searchsorted(ax, hi, side="left")), len(ax) - 1)  # cells i0 .. i1 - 1
    slope = np.diff(den, axis=1) / np.diff(ax)[None, :]
    inner = slice(i0, i1 - 1)  # jumps between cells k and k + 1, k = i0 .. i1 - 2, sit at node k + 1
    rel_jump = (np.abs(np.diff(slope, axis=1))[:, inner] / np.abs(den[:, 1:-1][:, inner])).max() if i1 - i0 > 1 else 0.0
    cells = slice(i0, i1)
    rel_slope = (np.abs(slope[:, cells]) / np.minimum(np.abs(den[:, 1:]), np.abs(den[:, :-1]))[:, cells]).max()
    step = np.abs(np.diff(el)).max()
    d4 = np.abs(np.diff(el, n=4)).max()
    # Samples BEFORE the first knot (none in the reference, whose coarse grid starts at the first sample) would be
    # EXTRAPOLATED by both forms, and the cubic's error on g at a distance
    # delta h beyond the end is delta (delta+1) (delta+2) (delta+3) / 24 times h^4 d4g/dt4 -- 0.95 at delta = 1
    # against the 5/384 of an interior interval -- and a kink there is missed by delta x (slope jump) x h.  (A
    # randomised sweep found the form 9e-5 off in the last four samples of a tight, fast scan: a 0.13 deg daisy
    # at 0.6 deg/s, 12 knots per turn.)
    t, ta = np.asarray(t, float), np.asarray(ta, float)
    h = (ta[-1] - ta[0]) / max(len(ta) - 1, 1)
    delta = max(0.0, (ta[0] - t.min()) / h) if len(t) else 0.0  # (past the last knot the samples are divided one by one)
    smooth = max(5.0 / 384.0, delta * (delta + 1) * (delta + 2) * (delta + 3) / 24.0)
    kink = max(SPLINE_KINK, delta)
    # + 4e-7: the two forms round differently in float32 (and the per-sample writer interpolates
    # the reciprocal over 4 samples)
    return float(1.1 * (kink * rel_jump * step + smooth * rel_slope * d4) + 4e-7)
