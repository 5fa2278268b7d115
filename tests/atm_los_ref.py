"""Every atmosphere sample's cell and weight against an exact line of sight.  Plain numpy, no torch.

The position of every (detector, coarse step, layer) on the layer's grid, in pixels, evaluated in numpy.longdouble with no
rounding between the steps, on the numbers the device receives; two float32 restatements of the unit projection (the
oracle's and the pixel kernel's own form); the radius eps per layer that separates a float32 evaluation from the exact one;
the screens that turn a position error into a value error at full size (index ramps, triangle waves, white noise) with the
value bounds that follow from eps; the band lookup in float64; and a numpy model of the pixel kernel's anchor + delta
arithmetic, on which tests/test_host_atm_los_ref.py sizes the mutations of DESIGN 3.41 against eps.  Nothing in this file is
measured on the device.  tests/test_gpu_atm_los.py holds the kernels to it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
f32 = np.float32
U24 = 2.0 ** -24
EPS_CAP = 5e-3  # pixels: a (case, layer) of the pixel route whose eps is larger is not sharp enough to be a test
MARGIN = 3.0    # the device's chain is another float32 evaluation (OCML: 1-2 ulp sin/cos/atan2/asin, 1-ulp div_near; numpy: 1 ulp)
HALF_PI_F32 = f32(1.57079637050628662109375)  # kHalfPiF of mrx_sample_px.h
N_DET = 300     # 256 + 44 live lanes in the second detector block
PWV0 = 1.0
TRI_PERIOD, TRI_PEAK = 16, 8.0
TRI_RMS, RAMP_RMS = 2.0 ** -1, 2.0 ** -6  # pwv stays inside the band tables' 0 ... 10 mm: 1 + 8/2, 1 + 511/64


# ---- the exact line of sight ----


def _unit(dx, dy, az, el, ft=LD):
    """(px, py, theta) [D, Ta] in ``ft``: transforms.py:10-29 as pointing_ref.exact_offsets step 1 states them, then the
    unit-height ground projection (px, py) = (re cos az - Y sin az, Y cos az + re sin az) / im; theta = asin(im).  pi / 2 is
    ``ft``'s own, not the float32 constant of the chain."""
    half_pi = np.arccos(ft(0))
    dx, dy = np.asarray(dx).astype(ft)[:, None], np.asarray(dy).astype(ft)[:, None]
    az, el = np.asarray(az).astype(ft)[None, :], np.asarray(el).astype(ft)[None, :]
    r = np.sqrt(dx * dx + dy * dy)
    p = np.arctan2(-dx, -dy)
    A, Y, cr = np.sin(r) * np.cos(p), np.sin(r) * np.sin(p), np.cos(r)
    a = el - half_pi
    re, im = A * np.cos(a) - cr * np.sin(a), A * np.sin(a) + cr * np.cos(a)
    return (re * np.cos(az) - Y * np.sin(az)) / im, (Y * np.cos(az) + re * np.sin(az)) / im, np.arcsin(im)


def device_inputs(problem):
    """(dx, dy, az, el) as the float32 numbers the device receives."""
    off = np.asarray(problem["offsets"], float)
    return f32(off[:, 0]), f32(off[:, 1]), f32(np.asarray(problem["az_a"])), f32(np.asarray(problem["el_a"]))


def exact_unit(problem, ft=LD):
    """(px, py, theta) [D, Ta] of every detector, and of the boresight [1, Ta], on the device's float32 inputs."""
    dx, dy, az, el = device_inputs(problem)
    return _unit(dx, dy, az, el, ft), _unit(np.zeros(1), np.zeros(1), az, el, ft)


def axis_hint(axis):
    """(g0, dg) of DevicePath._make_plan: the float64 grid behind the float32 axis, the step from the whole span."""
    ax = np.asarray(axis, float)
    return float(ax[0]), float((ax[-1] - ax[0]) / (len(ax) - 1))


def axis_is_uniform(axis):
    """plan_finish_layers' rule: every float32 node within an ulp of float32(g0 + i dg)."""
    g0, dg = axis_hint(axis)
    node = f32(np.asarray(axis))
    a = f32(np.arange(len(node)) * dg + g0)
    tol = np.maximum(np.maximum(np.abs(a), np.abs(node)), f32(abs(dg))) * f32(2.0 ** -23)
    return bool(dg > 0 and (np.abs(a - node) <= tol).all())


def _place(x, axis, uniform):
    """x (longdouble, metres) on the axis, in pixels: (x - g0) / dg on a uniform one; on any other the cell by exact search
    among the float32 nodes the device holds (jax's rule: clip(searchsorted(left) - 1, 0, n - 2)) plus the fraction inside."""
    if uniform:
        g0, dg = axis_hint(axis)
        return (x - LD(g0)) / LD(dg)
    nodes = f32(np.asarray(axis)).astype(LD)
    i = np.clip(np.searchsorted(nodes, x.ravel(), side="left").reshape(x.shape) - 1, 0, len(nodes) - 2)
    return i + (x - nodes[i]) / (nodes[i + 1] - nodes[i])


@dataclass(frozen=True)
class Position:
    pos: np.ndarray        # [L, D, Ta, 2] float64: (along the extrusion axis, across) in pixels
    bore: np.ndarray       # [L, Ta, 2]: the boresight's own line of sight
    theta: np.ndarray      # [D, Ta] float64: the exact elevation asin(im)
    unit: tuple            # (px, py) [D, Ta] longdouble
    pixel: tuple           # per layer: both axes verified uniform (the pixel route applies)
    shape: tuple           # per layer: (n_e, n_c)
    res: np.ndarray        # per layer: the smallest node spacing of either axis, metres
    metres: np.ndarray     # per layer: the largest |coordinate| in metres of any sample or node
    delta: np.ndarray      # per layer: the largest exact distance in pixels of a sample from its step's boresight position


def exact_position(problem):
    """The position of every (detector, coarse step, layer) on the layer's grid and the exact theta: longdouble throughout,
    on the float32 az_a, el_a, dx, dy, the float64 h, transform, axes and the wind offsets of oracle.hotpath.layer_offsets.
    h (px, py, 1) plus the wind translation, times transform, placed on the axes."""
    from oracle import hotpath

    (px, py, theta), (bx, by, _) = exact_unit(problem)
    pos, bore, pixel, shape, res, metres, delta = [], [], [], [], [], [], []
    for layer in problem["layers"]:
        oe, oc = (np.asarray(o).astype(LD)[None, :] for o in hotpath.layer_offsets(layer, problem["timestep"]))
        R, h = np.asarray(layer["transform"], float).astype(LD), LD(layer["h"])
        uni = axis_is_uniform(layer["extrusion"]) and axis_is_uniform(layer["cross_section"])
        out = []
        for x, y in ((px, py), (bx, by)):
            xe, xc = h * (x * R[0, 0] + y * R[1, 0]) + oe, h * (x * R[0, 1] + y * R[1, 1]) + oc
            out.append((np.stack([_place(xe, layer["extrusion"], uni), _place(xc, layer["cross_section"], uni)], axis=-1), xe, xc))
        (p, xe, xc), (b, _, _) = out
        pos.append(p.astype(np.float64))
        bore.append(b[0].astype(np.float64))
        pixel.append(uni)
        shape.append((len(layer["extrusion"]), len(layer["cross_section"])))
        res.append(min(np.diff(np.asarray(layer["extrusion"], float)).min(), np.diff(np.asarray(layer["cross_section"], float)).min()))
        metres.append(max(float(np.abs(xe).max()), float(np.abs(xc).max()),
                          float(np.abs(layer["extrusion"]).max()), float(np.abs(layer["cross_section"]).max())))
        delta.append(float(np.hypot(*np.moveaxis((p - b).astype(np.float64), -1, 0)).max()))
    pos = np.stack(pos)
    pos.setflags(write=False)
    return Position(pos, np.stack(bore), theta.astype(np.float64), (px, py), tuple(pixel), tuple(shape), np.array(res, float),
                    np.array(metres), np.array(delta))


# ---- the two float32 restatements of the unit projection ----


def unit_oracle(problem):
    """(px, py, theta) through the oracle: hotpath.broadcast, then hotpath.project_unit."""
    from oracle import hotpath

    dx, dy, az, el = device_inputs(problem)
    phi, theta = hotpath.broadcast(np.stack([dx, dy], axis=1), az, el)
    pp = hotpath.project_unit(phi, theta)
    return pp[..., 0], pp[..., 1], theta


def unit_kernel(problem):
    """(px, py, theta, pcx, pcy) in the pixel kernel's own form (mrx_sample_px.h, px_sample_items: the boresight terms of the
    item's prologue, the per-detector constants, the per-step projection), every operation rounded to float32.  pcx, pcy
    [Ta]: the boresight's own projection, which the anchors are made from and the lanes subtract."""
    dx, dy, az, el = device_inputs(problem)
    a = el - HALF_PI_F32
    ca, sa, cz, sz = np.cos(a), np.sin(a), np.cos(az), np.sin(az)
    pcx, pcy = (-sa * cz) / ca, (-sa * sz) / ca
    dx, dy = dx[:, None], dy[:, None]
    r = np.sqrt(dx * dx + dy * dy)
    p = np.arctan2(-dx, -dy)
    sr, cr = np.sin(r), np.cos(r)
    A, Y = sr * np.cos(p), sr * np.sin(p)
    re, im = A * ca - cr * sa, A * sa + cr * ca
    inv_im = f32(1) / im
    px, py = (re * cz - Y * sz) * inv_im, (Y * cz + re * sz) * inv_im
    assert px.dtype == f32 and pcx.dtype == f32
    return px, py, np.arcsin(im), pcx, pcy


def unit_errors(problem, exact):
    """{restatement: (largest distance of (px, py) from the exact projection, largest |theta - exact theta|)}."""
    ex, ey = exact.unit
    out = {}
    for name, (px, py, th) in (("oracle", unit_oracle(problem)), ("kernel", unit_kernel(problem)[:3])):
        out[name] = (float(np.hypot((px.astype(LD) - ex).astype(float), (py.astype(LD) - ey).astype(float)).max()),
                     float(np.abs(th.astype(np.float64) - exact.theta).max()))
    return out


# ---- the screens and what a position error does to them ----


def tri(x):
    """The triangle wave of period 16 nodes, values 0 ... 8, kinks on nodes: slope +-1 per pixel."""
    return TRI_PEAK - np.abs(np.mod(x, TRI_PERIOD) - TRI_PEAK)


def axis_screen(shape, axis, kind):
    """float32 [n_e, n_c]: the index ramp v[i][j] = i (axis 0) or j (axis 1), or the triangle wave of that index."""
    idx = np.arange(shape[axis], dtype=np.float64)
    line = idx if kind == "ramp" else tri(idx)
    return np.ascontiguousarray(np.broadcast_to(line[:, None] if axis == 0 else line[None, :], shape), f32)


def axis_value(x, kind):
    """What a bilinear blend of axis_screen gives at position x along that axis (exact: linear between the nodes)."""
    return x if kind == "ramp" else tri(x)


def noise_screens(shapes, seed=20260):
    """White noise: float32 N(0, 1), one screen per layer, from a fixed seed."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s, dtype=f32) for s in shapes]


def _cell(x, n):
    i = np.clip(np.floor(x), 0, n - 2).astype(np.int64)
    return i, x - i


def bilinear(v, pos):
    """The float64 bilinear blend of screen v at positions pos [..., 2] (cells clamped onto the grid)."""
    v = np.asarray(v, np.float64)
    (i, we), (j, wc) = _cell(pos[..., 0], v.shape[0]), _cell(pos[..., 1], v.shape[1])
    y0 = v[i, j] + wc * (v[i, j + 1] - v[i, j])
    y1 = v[i + 1, j] + wc * (v[i + 1, j + 1] - v[i + 1, j])
    return y0 + we * (y1 - y0)


def lipschitz(v, pos):
    """L(x): the largest |difference of edge-adjacent nodes| over the cells within one pixel of x (the cell of x and its
    eight neighbours).  A bilinear surface is continuous, and Lipschitz with that constant along either axis."""
    v = np.asarray(v, np.float64)
    de, dc = np.abs(np.diff(v, axis=0)), np.abs(np.diff(v, axis=1))  # [n_e-1, n_c], [n_e, n_c-1]
    cell = np.maximum(np.maximum(de[:, :-1], de[:, 1:]), np.maximum(dc[:-1, :], dc[1:, :]))  # [n_e-1, n_c-1]
    pad = np.pad(cell, 1, mode="edge")
    near = cell
    for a in range(3):
        for b in range(3):
            near = np.maximum(near, pad[a:a + cell.shape[0], b:b + cell.shape[1]])
    i, _ = _cell(pos[..., 0], v.shape[0])
    j, _ = _cell(pos[..., 1], v.shape[1])
    return near[i, j]


def layer_bound(v, pos, eps):
    """eps L(x) + r per sample: r = 3 2^-24 max|corner|, the float32 rounding of one layer's blend (two lerps and one)."""
    return eps * lipschitz(v, pos) + 3 * U24 * float(np.abs(v).max())


def stack_reference(pos, screens, rms, eps):
    """(sum_l rms_l y_l, bound) [D, Ta] of the whole stack at the exact positions: the float64 blends, and the summed layer
    bounds plus n_layers 2^-24 sum_l |rms_l y_l| for the float32 accumulation in layer order."""
    total, bound, mag = 0.0, 0.0, 0.0
    for l, v in enumerate(screens):
        r = float(f32(rms[l]))
        y = bilinear(v, pos[l])
        total = total + r * y
        bound = bound + r * layer_bound(v, pos[l], eps[l])
        mag = mag + np.abs(r * y)
    return total, bound + len(screens) * U24 * mag


def rim_margin(pos, shapes):
    """[L, D, Ta]: how far inside its layer's grid a position lies, in pixels (negative: beyond a rim), and per side
    [L, 4, D, Ta] (extrusion first, extrusion last, cross first, cross last)."""
    sides = np.stack([np.stack([pos[l, ..., 0], (s[0] - 1) - pos[l, ..., 0], pos[l, ..., 1], (s[1] - 1) - pos[l, ..., 1]])
                      for l, s in enumerate(shapes)])
    return sides.min(axis=1), sides


def rim_classes(pos, shapes, eps):
    """(must_nan, must_be_finite) [D, Ta]: some layer's exact position lies beyond the grid by more than eps; every layer's
    lies inside by more than eps.  In the band between, either outcome passes."""
    m, _ = rim_margin(pos, shapes)
    e = np.asarray(eps)[:, None, None]
    return (m < -e).any(axis=0), (m > e).all(axis=0)


# ---- the band lookup ----


def band_reference(problem, pwv_dev, theta, e_theta):
    """(P, bound) [D, Ta]: the float64 trilinear evaluation of each detector's band table (the float32 values and axes the
    device holds, the float32 temperature weight of pipeline_host.table_slabs) at the device's own pwv rounded to float32 and
    the exact theta, times the Mueller weight; bound = 12 2^-24 |P| + |dP/dtheta| 3 e_theta, the slope from the table cell."""
    from maria_amd.pipeline_host import table_slabs

    xp_all = f32(pwv_dev).astype(np.float64)
    P, bound = np.full(theta.shape, np.nan), np.full(theta.shape, np.nan)
    band, m00 = np.asarray(problem["band_index"]), np.asarray(problem["m00"], np.float64)
    for b, table in enumerate(problem["tables"]):
        rows = np.flatnonzero(band == b)
        if len(rows) == 0:
            continue
        vals, w_t, oob = table_slabs(table, problem["T0"])
        assert not oob
        s = (1.0 - float(w_t)) * vals[0].astype(np.float64) + float(w_t) * vals[1].astype(np.float64)  # [n_pwv, n_el]
        axp, axe = f32(table["pwv"]).astype(np.float64), f32(table["el"]).astype(np.float64)
        xp, xe = xp_all[rows], np.minimum(theta[rows], float(HALF_PI_F32))
        ip = np.clip(np.searchsorted(axp, xp, side="left") - 1, 0, len(axp) - 2)
        ie = np.clip(np.searchsorted(axe, xe, side="left") - 1, 0, len(axe) - 2)
        wp, we = (xp - axp[ip]) / (axp[ip + 1] - axp[ip]), (xe - axe[ie]) / (axe[ie + 1] - axe[ie])
        lo = (1 - wp) * s[ip, ie] + wp * s[ip + 1, ie]
        hi = (1 - wp) * s[ip, ie + 1] + wp * s[ip + 1, ie + 1]
        val = m00[rows, None] * (lo + we * (hi - lo))
        slope = m00[rows, None] * (hi - lo) / (axe[ie + 1] - axe[ie])
        P[rows], bound[rows] = val, 12 * U24 * np.abs(val) + np.abs(slope) * 3 * e_theta
    return P, bound


def band_model(problem, pwv_dev, theta32, mutation=None):
    """band_loading_px in numpy: the cell by search, the weights in float32 (div_near: the quotient; ``mutation`` 8: c.w taken
    as (x - lo) * inv with the axis' first step), the 8-term sum in float64.  [D, Ta]."""
    from maria_amd.pipeline_host import table_slabs

    out = np.full(theta32.shape, np.nan)
    band = np.asarray(problem["band_index"])
    for b, table in enumerate(problem["tables"]):
        rows = np.flatnonzero(band == b)
        if len(rows) == 0:
            continue
        vals, w_t, _ = table_slabs(table, problem["T0"])
        s = (1.0 - float(w_t)) * vals[0].astype(np.float64) + float(w_t) * vals[1].astype(np.float64)
        w, idx = [], []
        for ax, x in ((f32(table["pwv"]), f32(pwv_dev)[rows]), (f32(table["el"]), np.minimum(f32(theta32)[rows], HALF_PI_F32))):
            i = np.clip(np.searchsorted(ax, x, side="left") - 1, 0, len(ax) - 2)
            inv = f32(1) / (ax[1] - ax[0])
            w.append(((x - ax[i]) * inv if mutation == 8 else (x - ax[i]) / (ax[i + 1] - ax[i])).astype(np.float64))
            idx.append(i)
        (ip, ie), (wp, we) = idx, w
        lo = (1 - wp) * s[ip, ie] + wp * s[ip + 1, ie]
        hi = (1 - wp) * s[ip, ie + 1] + wp * s[ip + 1, ie + 1]
        out[rows] = np.asarray(problem["m00"], np.float64)[rows, None] * (lo + we * (hi - lo))
    return out


# ---- a numpy model of the pixel kernel: anchor + delta, the range-checked gathers, the float32 blend ----


def _fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 numbers is exact in float64."""
    return f32(a.astype(np.float64) * np.float64(b) + np.asarray(c, np.float64))


def pixel_model(problem, screens, rms=None, mutation=None, kt=1, pipe=False, stages=3):
    """The pwv [D, Ta] float64 (NaN off a screen) that px_sample_items' arithmetic gives, operation by operation in float32
    where the kernel's is, and the positions it took [L, D, Ta, 2] (cell + weight).  ``mutation``: one of DESIGN 3.41's
    1 ... 7 (6 needs ``pipe``, 7 ``kt`` = 2); the unmutated model is itself held to the bounds on the CPU."""
    from oracle import hotpath

    px, py, _, pcx, pcy = unit_kernel(problem)
    dpx, dpy = px - pcx[None, :], py - pcy[None, :]
    Ta = len(pcx)
    steps = np.arange(Ta)
    if mutation == 5:
        steps = np.maximum(steps - 1, 0)
    if mutation == 7 and kt == 2:
        steps = steps - (steps & 1)  # (an even chunk: the pairs start on even steps)
    n_layers = len(screens)
    rms = [l["pwv_rms"] for l in problem["layers"]] if rms is None else rms
    stage = []
    for l, (layer, v) in enumerate(zip(problem["layers"], screens)):
        n_e, n_c = v.shape
        (e0, de), (c0, dc) = axis_hint(layer["extrusion"]), axis_hint(layer["cross_section"])
        R, h = np.asarray(layer["transform"], float), float(layer["h"])
        pe_x, pe_y, pc_x, pc_y = h * R[0, 0] / de, h * R[1, 0] / de, h * R[0, 1] / dc, h * R[1, 1] / dc
        oe, oc = hotpath.layer_offsets(layer, problem["timestep"])
        ox, oy = ((oe - e0) / de)[steps], ((oc - c0) / dc)[steps]
        bx, by = pcx[steps], pcy[steps]
        if mutation == 1:
            Fe = (bx * f32(pe_x) + (by * f32(pe_y) + f32(ox))).astype(np.float64)
            Fc = (bx * f32(pc_x) + (by * f32(pc_y) + f32(oy))).astype(np.float64)
        else:
            Fe = bx.astype(np.float64) * pe_x + (by.astype(np.float64) * pe_y + ox)
            Fc = bx.astype(np.float64) * pc_x + (by.astype(np.float64) * pc_y + oy)
        ce, cc = np.floor(Fe), np.floor(Fc)
        mid_e, mid_c = f32(0.5 * (n_e - 1) - ce), f32(0.5 * (n_c - 1) - cc)
        fe = _fma32(dpx, f32(pe_x), _fma32(dpy, f32(pe_y), f32(Fe - ce)[None, :]))
        fc = _fma32(dpx, f32(pc_x), _fma32(dpy, f32(pc_y), f32(Fc - cc)[None, :]))
        half_e = f32(n_e / 2) if mutation == 4 else f32(0.5) * f32(n_e - 1)
        half_c = f32(0.5) * f32(n_c - 1)
        outside = ~(np.abs(fe - mid_e[None, :]) <= half_e) | ~(np.abs(fc - mid_c[None, :]) <= half_c)
        we, wc = fe - np.floor(fe), fc - np.floor(fc)
        ie, ic = ce[None, :].astype(np.int64) + np.floor(fe).astype(np.int64), cc[None, :].astype(np.int64) + np.floor(fc).astype(np.int64)
        flat = np.concatenate([v.ravel(), np.zeros(1, f32)])  # (a gather beyond the screen's range reads zero)

        def gather(k):
            return flat[np.where((k >= 0) & (k < n_e * n_c), k, n_e * n_c)]

        k0 = ie * n_c + ic
        r0x, r0y, r1x, r1y = gather(k0), gather(k0 + 1), gather(k0 + n_c), gather(k0 + n_c + 1)
        if mutation == 2:
            r0y, r1x = r1x, r0y
        if mutation == 3:
            we, wc = wc, we
        stage.append(dict(r0x=r0x, r0y=r0y, r1x=r1x, r1y=r1y, we=f32(we), wc=f32(wc), rms=f32(rms[l]), outside=outside,
                          pos=np.stack([ie + we.astype(np.float64), ic + wc.astype(np.float64)], axis=-1)))
    fl = np.zeros(dpx.shape, f32)
    outside = np.zeros(dpx.shape, bool)
    zero = dict(stage[0], r0x=f32(0), r0y=f32(0), r1x=f32(0), r1y=f32(0), rms=f32(0))
    for l in range(n_layers):
        g = stage[l]
        outside |= g["outside"]
        if mutation == 6 and pipe:  # the ring's next slot: the layer after, or what an earlier layer left there
            k = l + 1 if l + 1 < n_layers else l + 1 - stages
            g = stage[k] if k >= 0 else zero
        y0 = _fma32(g["wc"], g["r0y"] - g["r0x"], g["r0x"])
        y1 = _fma32(g["wc"], g["r1y"] - g["r1x"], g["r1x"])
        fl = _fma32(_fma32(g["we"], y1 - y0, y0), g["rms"], fl)
    pwv = np.where(outside | np.isnan(fl), np.nan, float(problem["pwv0"]) + fl.astype(np.float64))
    return pwv, np.stack([g["pos"] for g in stage])


def literal_model(problem):
    """The positions [L, D, Ta, 2] of the literal route (MRX_OPT_AXIS_LITERAL; atm_sample_kernel's array search): the float32
    coordinate of the float64 sum, the cell among the float32 nodes, the float32 quotient as weight."""
    from oracle import hotpath

    px, py, _, _, _ = unit_kernel(problem)
    px, py = px.astype(np.float64), py.astype(np.float64)
    out = []
    for layer in problem["layers"]:
        R, h = np.asarray(layer["transform"], float), float(layer["h"])
        oe, oc = hotpath.layer_offsets(layer, problem["timestep"])
        p = []
        for x, ax in ((f32(px * (h * R[0, 0]) + (py * (h * R[1, 0]) + oe[None, :])), f32(np.asarray(layer["extrusion"]))),
                      (f32(px * (h * R[0, 1]) + (py * (h * R[1, 1]) + oc[None, :])), f32(np.asarray(layer["cross_section"])))):
            i = np.clip(np.searchsorted(ax, x.ravel(), side="left").reshape(x.shape) - 1, 0, len(ax) - 2)
            p.append(i + ((x - ax[i]) / (ax[i + 1] - ax[i])).astype(np.float64))
        out.append(np.stack(p, axis=-1))
    return np.stack(out)


# ---- the cases ----


def stretched_table():
    """A band table whose pwv and elevation axes are not uniform (synthetic.emission_tables' second band on stretched
    nodes): guess_cell's first-step guess misses, and a weight taken with the first step's inverse is wrong at full size."""
    T = np.array([250.0, 270.0, 290.0])
    u = np.linspace(0.0, 1.0, 32)
    pwv = 10.0 * u * (1.0 + 0.6 * u) / 1.6
    el = np.radians(10.0 + 80.0 * u * (1.0 + 0.4 * u) / 1.4)
    el[-1] = np.radians(90.1)
    a, tau0, kappa = 30.0, 0.04, 0.025
    tau = (tau0 + kappa * pwv[None, :, None]) / np.sin(np.minimum(el, np.pi / 2))[None, None, :]
    return {"T": T, "pwv": pwv, "el": el, "values": a * (T[:, None, None] / 270.0) * (1.0 - np.exp(-tau))}


def footprint(problem, layer, fov_deg):
    """(e, c): the coordinates in metres, along the layer's two axes, of the points synthetic.make_problem sizes a screen by
    (the boresight and a ring at 1.02 of the field's edge, every coarse step)."""
    from maria_amd import synthetic

    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    ring = 0.5 * np.radians(fov_deg) * 1.02 * np.c_[np.cos(ang), np.sin(ang)]
    phi, theta = synthetic._pointing_f64(np.r_[np.zeros((1, 2)), ring], np.asarray(problem["az_a"]), np.asarray(problem["el_a"]))
    px, py = np.cos(phi) / np.tan(theta), np.sin(phi) / np.tan(theta)
    h, ts = layer["h"], problem["timestep"]
    ce, se = layer["transform"][0, 0], layer["transform"][1, 0]
    tx, ty = np.cumsum(ts * layer["vx"]), np.cumsum(ts * layer["vy"])
    return (h * px + tx[None]) * ce + (h * py + ty[None]) * se, -(h * px + tx[None]) * se + (h * py + ty[None]) * ce


def _set_axes(layer, e, c, res, n_e, n_c, shift=(0.0, 0.0)):
    """start + i * step about the footprint's middle, as make_problem builds them; ``shift`` in pixels."""
    layer["extrusion"] = (0.5 * (e.min() + e.max()) - 0.5 * res * (n_e - 1) + shift[0] * res) + res * np.arange(n_e)
    layer["cross_section"] = (0.5 * (c.min() + c.max()) - 0.5 * res * (n_c - 1) + shift[1] * res) + res * np.arange(n_c)
    layer["res"] = float(res)


F_SHIFT = 31.0e3  # metres along each axis: the float32 coordinate is spaced 2^-9 m there, 3.9e-4 of a 5-m pixel
R_RES, R_CROP, R_SHIFT = 0.5, 0.9, (0.37, -0.21)
L_EXTRA = 6000    # nodes upstream of the footprint: the position along the extrusion axis is 6000 ... 6127 pixels, spaced 4.9e-4 in float32


def _make(name):
    from maria_amd import synthetic

    geo = dict(n_det=N_DET, n_bands=2, fs=50.0, duration=20.1, t0=1.7e9, pwv0=PWV0)
    fov, side = (2.0, 512) if name == "W" else (0.5, 128)
    n_layers = {"S": 7, "W": 8, "F": 3, "R": 2, "N": 3, "L": 3}[name]
    p = synthetic.make_problem(fov_deg=fov, side=side, n_layers=n_layers, min_res=5.0, **geo)
    if name != "S":
        p["tables"] = [p["tables"][0], stretched_table()]
    if name == "F":
        for layer in p["layers"]:
            ce, se = layer["transform"][0, 0], layer["transform"][1, 0]
            layer["vx"], layer["vy"] = layer["vx"].copy(), layer["vy"].copy()
            layer["vx"][0] += (ce * F_SHIFT - se * F_SHIFT) / p["timestep"]
            layer["vy"][0] += (se * F_SHIFT + ce * F_SHIFT) / p["timestep"]
            e, c = footprint(p, layer, fov)
            res = max(5.0, max(np.ptp(e), np.ptp(c)) * 1.02 / (side - 8))
            _set_axes(layer, e, c, res, side, side)
    if name == "L":
        for layer in p["layers"]:
            e, c = footprint(p, layer, fov)
            _set_axes(layer, e, c, 5.0, side + L_EXTRA, side, (-0.5 * L_EXTRA, 0.0))
    if name == "R":
        for layer in p["layers"]:
            e, c = footprint(p, layer, fov)
            n_e, n_c = int(np.floor(R_CROP * np.ptp(e) / R_RES)) + 1, int(np.floor(R_CROP * np.ptp(c) / R_RES)) + 1
            _set_axes(layer, e, c, R_RES, n_e, n_c, R_SHIFT)
    if name == "N":  # as tests/test_gpu_parity.py::test_nonuniform_axes_take_the_array_path
        ax = p["layers"][1]["cross_section"]
        mid = 0.5 * (ax[0] + ax[-1])
        p["layers"][1]["cross_section"] = mid + (ax - mid) * (1.0 + 0.3 * ((ax - mid) / (ax[-1] - mid)) ** 2)
        ex = p["layers"][2]["extrusion"].copy()
        ex[len(ex) // 2] += 0.4 * (ex[1] - ex[0])
        p["layers"][2]["extrusion"] = ex
    assert len(p["ta"]) % 2 == 1, "Ta odd: the last pair of steps straddles the end"
    return p


@dataclass
class Case:
    name: str
    fov_deg: float = field(init=False)

    def __post_init__(self):
        self.fov_deg = 2.0 if self.name == "W" else 0.5

    @functools.cached_property
    def problem(self):
        """Geometry and tables; the layers carry no screens (the tests bind their own)."""
        return _make(self.name)

    @functools.cached_property
    def exact(self):
        return exact_position(self.problem)

    @functools.cached_property
    def errors(self):
        return unit_errors(self.problem, self.exact)

    @property
    def e_unit(self):
        return max(e[0] for e in self.errors.values())

    @property
    def e_theta(self):
        return max(e[1] for e in self.errors.values())

    @property
    def h_over_res(self):
        return np.array([l["h"] for l in self.problem["layers"]]) / self.exact.res

    def eps(self, route="pixel"):
        """Per layer, in pixels: 3 E_unit h / res + 4 2^-24 max|delta| (the two float32 fused multiply-adds of the delta per
        axis).  ``route`` "literal" (MRX_OPT_AXIS_LITERAL, MRX_OPT_POINTING_CHAIN) adds, on every layer, the float32 spacing
        of the largest |coordinate in metres| over res: the rounding of the reference's own coordinate, which those routes
        carry on purpose; "general" (atm_sample_kernel's default rule) adds it on the layers whose axes are searched as
        arrays."""
        e = MARGIN * self.e_unit * self.h_over_res + 4 * U24 * self.exact.delta
        spacing = np.array([float(np.spacing(f32(m))) for m in self.exact.metres]) / self.exact.res
        if route == "literal":
            return e + spacing
        if route == "general":
            return e + np.where(self.exact.pixel, 0.0, spacing)
        assert route == "pixel"
        return e

    @property
    def shapes(self):
        return self.exact.shape

    @functools.cached_property
    def noise(self):
        return noise_screens(self.shapes)

    def with_tables(self, n_pwv, n_el):
        """The same problem with band tables of n_pwv x n_el nodes (a shallow copy: the geometry is shared)."""
        from maria_amd import synthetic

        return dict(self.problem, tables=synthetic.emission_tables(len(self.problem["tables"]), n_pwv=n_pwv, n_el=n_el))


# ---- the checks: every sample of a run, against the exact positions ----


class Judge:
    """What a run of a case through a route is held to.  ``route``: which eps (Case.eps).  tests/test_gpu_atm_los.py hands
    it what the device wrote; tests/test_host_atm_los_ref.py what pixel_model gives, mutated and not."""

    def __init__(self, case, route="pixel"):
        self.case, self.eps = case, case.eps(route)
        self.must_nan, self.must_be_finite = rim_classes(case.exact.pos, case.shapes, self.eps)
        self.profile = [l["pwv_rms"] for l in case.problem["layers"]]
        self.worst = dict(position=0.0, stack=0.0, band=0.0)

    def rim(self, pwv):
        """NaN exactly where some layer's exact position lies beyond its grid by more than eps; finite where every layer's
        lies inside by more than eps."""
        assert np.isnan(pwv[self.must_nan]).all(), "a sample beyond a rim came out finite"
        assert np.isfinite(pwv[self.must_be_finite]).all(), "a sample inside every grid came out NaN"

    def band(self, problem, pwv, loading):
        """The band lookup at the run's own pwv and the exact theta: guess_cell, div_near and the 8-term sum."""
        assert np.array_equal(np.isnan(loading), np.isnan(pwv))
        P, bound = band_reference(problem, pwv, self.case.exact.theta, self.case.e_theta)
        ok = np.isfinite(pwv)
        ratio = float((np.abs(np.asarray(loading, np.float64) - P)[ok] / bound[ok]).max())
        self.worst["band"] = max(self.worst["band"], ratio)
        assert ratio <= 1.0, f"band lookup: |loading - P| / bound = {ratio:.3f}"

    def axis(self, l, axis, kind, pwv):
        """Layer l alone, lit at a power of two, on the ramp or the triangle wave along ``axis``: every sample's
        |pwv - pwv0 - rms v(x_exact)| <= rms (eps + r), no allowance."""
        self.rim(pwv)
        rms = RAMP_RMS if kind == "ramp" else TRI_RMS
        vmax = float(axis_screen(self.case.shapes[l], axis, kind).max())
        got = (pwv - PWV0) / rms  # exact: rms is a power of two and pwv0 + (double)fl is exact
        want = axis_value(self.case.exact.pos[l, ..., axis], kind)
        r = 3 * U24 * vmax
        err = np.abs(got - want)
        inside = self.must_be_finite
        worst = float(err[inside].max())
        if kind == "tri":
            self.worst["position"] = max(self.worst["position"], worst)
        assert worst <= self.eps[l] + r, f"layer {l} axis {axis} {kind}: {worst:.3e} pixel > eps {self.eps[l]:.3e} + {r:.1e}"
        band = np.isfinite(pwv) & ~inside  # within eps of a rim and finite: a cell that hangs over the rim
        assert (err[band] <= self.eps[l] * 2 * vmax + r).all()

    def stack(self, pwv, screens=None):
        """The whole stack lit at the profile's pwv_rms on white noise: every sample within the summed bound of the float64
        blends at the exact positions."""
        self.rim(pwv)
        screens = self.case.noise if screens is None else screens
        ref, bound = stack_reference(self.case.exact.pos, screens, self.profile, self.eps)
        err = np.abs(pwv - PWV0 - ref)
        inside = self.must_be_finite
        ratio = float((err[inside] / bound[inside]).max())
        self.worst["stack"] = max(self.worst["stack"], ratio)
        assert ratio <= 1.0, f"white-noise stack: |pwv - ref| / bound = {ratio:.3f}"
        band = np.isfinite(pwv) & ~inside
        over = sum(float(f32(r)) * e * 2 * float(np.abs(v).max()) for r, e, v in zip(self.profile, self.eps, screens))
        assert (err[band] <= bound[band] + over).all()

    def axis_run(self, l, axis, kind):
        """(screens, amplitudes) of axis(): zeros everywhere but layer l."""
        shapes = self.case.shapes
        screens, amp = [np.zeros(s, f32) for s in shapes], [0.0] * len(shapes)
        screens[l], amp[l] = axis_screen(shapes[l], axis, kind), RAMP_RMS if kind == "ramp" else TRI_RMS
        return screens, amp


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


CASE_NAMES = ("S", "W", "F", "R", "N", "L")
