"""The K_RJ division against an exact elevation and an exact lookup.  Plain numpy, float64, no torch.

mrx_krj.h divides every K_RJ field by den_band(el_det): el_det from the boresight elevation and the detector's offsets
(coords/transforms.py:14-28), den by jax's linear lookup on the band's elevation axis.  Here both are evaluated without
rounding between the steps on the float32 numbers the device receives (el_exact, den_exact); the allowance tol is a
function of these two alone; a numpy restatement of which form of krj_row a (tile, row) takes shows that every case is what
it says (it is not the reference); and the tables and cases are chosen so that a neighbouring cell, a dropped kink or a
microradian of elevation shows.  tests/test_host_krj_ref.py checks this module on the CPU, tests/test_gpu_krj_forms.py the
kernels against it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

GRANT = 1.0e-6           # rad: the project's own grant -- the gate of KrjSamples::curved, the hardware sine and cosine
ULP = 2.0**-24           # half a float32 ulp of a number in [1, 2)
TILE, PER_THREAD, TILE_DET = 1024, 4, 16
HALF_RANGE = np.float32(2.0e-2)   # kModelHalfRange
CELL_DEG = 2.1875        # the zigzag axis' step: (90 - 20) / 32, as test_gpu_calibration._cal_tables spaces 33 nodes
CURVATURE_GATE = 5.0e-7  # rad: kModelCurvature of mrx_krj.h, the model's own curvature estimate beyond which a row is exact
FORMS = ("lin", "kink", "exact", "sample", "curved")  # the codes of forms()
LIN, KINK, EXACT, SAMPLE, CURVED = range(5)


# ---- the reference ----


def el_exact(dx, dy, bore_el):
    """asin(sin r cos p sin a + cos r cos a), a = el_bore - pi/2, p = atan2(-dx, -dy) (coords/transforms.py:14-28) in
    float64 of the float32 inputs: [D, T]."""
    dx = np.asarray(dx, np.float32).astype(np.float64)[:, None]
    dy = np.asarray(dy, np.float32).astype(np.float64)[:, None]
    a = np.asarray(bore_el, np.float32).astype(np.float64)[None, :] - np.pi / 2
    r = np.hypot(dx, dy)
    p = np.arctan2(-dx, -dy)
    return np.arcsin(np.clip(np.sin(r) * np.cos(p) * np.sin(a) + np.cos(r) * np.cos(a), -1.0, 1.0))


def cell_of(axis, el):
    """jax's index rule: clip(searchsorted(axis, el, "left") - 1, 0, n - 2)."""
    axis = np.asarray(axis, np.float32).astype(np.float64)
    return np.clip(np.searchsorted(axis, el, side="left") - 1, 0, len(axis) - 2)


def den_in_cell(axis, values, el, i):
    """The line of cell i of the axis at el (inside the cell or not), linear weights in float64 on the float32 nodes."""
    x = np.asarray(axis, np.float32).astype(np.float64)
    y = np.asarray(values, np.float32).astype(np.float64)
    w = (el - x[i]) / (x[i + 1] - x[i])
    return y[i] * (1.0 - w) + y[i + 1] * w


def den_exact(axis, values, el):
    """den at el: jax's index rule and linear weights, NaN off the axis.  values [n] of one band."""
    x = np.asarray(axis, np.float32).astype(np.float64)
    den = den_in_cell(axis, values, el, cell_of(axis, el))
    return np.where((el < x[0]) | (el > x[-1]), np.nan, den)


def slopes(axis, values):
    x = np.asarray(axis, np.float32).astype(np.float64)
    y = np.asarray(values, np.float32).astype(np.float64)
    return np.diff(y) / np.diff(x)


def groups_of(a):
    """[D, T] -> [D, G, 4]: the four samples 4k .. 4k + 3 of a thread, the last group padded with the row's last sample
    (as the kernel clamps its loads)."""
    D, T = a.shape
    G = -(-T // PER_THREAD)
    pad = np.concatenate([a, np.repeat(a[:, -1:], G * PER_THREAD - T, axis=1)], axis=1)
    return pad.reshape(D, G, PER_THREAD)


def straddle(axis, values, el):
    """[D, T]: |g_{i+1} - g_i| x the elevation span of the thread's four samples where those four have a node of the axis
    between them (the chord form misses a kink there by design), else 0."""
    x = np.asarray(axis, np.float32).astype(np.float64)
    g = slopes(axis, values)
    e = groups_of(el)
    lo, hi = e.min(axis=-1), e.max(axis=-1)
    # the inner nodes in (lo, hi): node k separates cells k - 1 and k
    k0 = np.searchsorted(x, lo, side="right")  # first node > lo
    k1 = np.searchsorted(x, hi, side="left") - 1  # last node < hi
    out = np.zeros(lo.shape)
    for k in range(1, len(x) - 1):
        m = (k0 <= k) & (k <= k1)
        out[m] += abs(g[k] - g[k - 1]) * (hi - lo)[m]
    return np.repeat(out, PER_THREAD, axis=1)[:, : el.shape[1]]


def tol(axis, values, el, b_el, chord_ok=True):
    """(|g| B_el + straddle) / den + 3 2^-24 per sample: g the slope of el's cell, the larger of the two cells' where the
    sample is within B_el of a node; chord_ok [T]: where the chord form may be taken at all (the tiles below the gate of
    KrjSamples::curved), no straddle elsewhere.  NaN where the reference is."""
    g = np.abs(slopes(axis, values))
    i = cell_of(axis, el)
    lo_i = np.clip(cell_of(axis, el - b_el), 0, len(g) - 1)
    hi_i = np.clip(cell_of(axis, el + b_el), 0, len(g) - 1)
    gg = np.maximum(g[i], np.maximum(g[lo_i], g[hi_i]))
    return (gg * b_el + np.where(chord_ok, straddle(axis, values, el), 0.0)) / np.abs(den_exact(axis, values, el)) + 3 * ULP


def near_an_end(axis, el, b_el):
    """Samples within B_el of an end of the axis: exempt from the NaN-pattern comparison."""
    x = np.asarray(axis, np.float32).astype(np.float64)
    return (np.abs(el - x[0]) <= b_el) | (np.abs(el - x[-1]) <= b_el)


# ---- the tables ----


def _axis_nodes(lo_deg, hi_deg):
    """Nodes lo + 2.1875 i below hi, the last one moved 0.1 deg off the uniform step (as _cal_tables' 90.1)."""
    n = int(np.floor((hi_deg - lo_deg) / CELL_DEG + 1e-9)) + 1
    deg = lo_deg + CELL_DEG * np.arange(n)
    deg[-1] += 0.1
    return deg


def table(kind, lo_deg=20.0, hi_deg=90.0):
    """(axis [n] float32, values [2, n] float32) of one kind: "ramp3", "ramp200" (den = el on every node: a field of ones
    comes back as the device's own elevation), "zigzag" ((1 + 0.25 b)(1 + 0.01 (-1)^i): a neighbouring cell costs up to
    2e-2, the slopes stay near 0.5 / rad) and "nonuniform" (the zigzag on an axis whose steps vary threefold)."""
    nodes = _axis_nodes(lo_deg, hi_deg)
    if kind in ("ramp3", "ramp200"):
        n = 3 if kind == "ramp3" else 200
        axis = np.radians(np.linspace(nodes[0], nodes[-1], n)).astype(np.float32)
        return axis, np.stack([axis, axis])
    if kind == "nonuniform":
        steps = np.resize([2.0, 1.0, 3.0, 1.5, 2.5], len(nodes) - 1)  # the arithmetic guess is right, one high or one low
        nodes = nodes[0] + np.concatenate([[0.0], np.cumsum(steps)]) * (nodes[-1] - nodes[0]) / steps.sum()
    elif kind != "zigzag":
        raise ValueError(kind)
    axis = np.radians(nodes).astype(np.float32)
    zig = 1.0 + 0.01 * (-1.0) ** np.arange(len(axis))
    return axis, np.stack([(1.0 + 0.25 * b) * zig for b in range(2)]).astype(np.float32)


KINDS = ("ramp3", "ramp200", "zigzag", "nonuniform")


# ---- which form a (tile, row) takes: a restatement of krj_prologue / krj_stage_rows / set_linear_den ----


def tile_ranges(bore_el):
    """Per tile of 1024 samples: (lo, hi, ebm) float32 and whether some thread's four boresight elevations are not linear
    in the sample index to 1e-6 rad (KrjSamples::curved, in the kernel's own float32 operations)."""
    eb = np.asarray(bore_el, np.float32)
    T = len(eb)
    out = []
    for s0 in range(0, T, TILE):
        idx = np.minimum(s0 + np.arange(TILE), T - 1)
        e = eb[idx].reshape(-1, PER_THREAD)
        third = (e[:, 3] - e[:, 0]) * np.float32(1.0 / 3.0)
        ok = (np.abs(e[:, 1] - (e[:, 0] + third)) <= np.float32(1e-6)) & (np.abs(e[:, 2] - (np.float32(2) * third + e[:, 0])) <= np.float32(1e-6))
        lo, hi = e.min(), e.max()
        out.append((lo, hi, np.float32(0.5) * (lo + hi), bool((~ok).any())))
    return out


def chord_deviation(bore_el):
    """[T] float64: how far the two inner samples of a thread's four lie off the chord between the outer two, from the
    float32 input in float64; zero on the outer samples."""
    eb = np.asarray(bore_el, np.float32).astype(np.float64)
    e = groups_of(eb[None, :])[0]
    dev = np.zeros_like(e)
    for q in (1, 2):
        dev[:, q] = np.abs(e[:, q] - (e[:, 0] + (e[:, 3] - e[:, 0]) * q / 3.0))
    return dev.reshape(-1)[: len(eb)]


def forms(off, bore_el, axis, curvature_gate=None):
    """[n_tiles, D] codes (FORMS) of the form krj_row takes: restated in float64 from the kernel's conditions.
    curvature_gate: the model's own curvature estimate (second difference of its three points) x (hi - lo)^2 / 8 above
    which krj_stage_rows marks a row exact."""
    off = np.asarray(off, np.float32)
    x = np.asarray(axis, np.float32).astype(np.float64)
    z = 1.0 / np.diff(x)
    n = len(x)
    h = float(HALF_RANGE)
    dy = off[:, 1].astype(np.float64)
    out = []
    for lo, hi, ebm, curved in tile_ranges(bore_el):
        lo, hi, ebm = float(lo), float(hi), float(ebm)
        pts = np.array([ebm - h, ebm, ebm + h])
        e = el_exact(off[:, 0], off[:, 1], pts.astype(np.float32)) - pts[None, :]
        dm, slope = e[:, 1], (e[:, 2] - e[:, 0]) * (0.5 / h)
        steep = (np.cos(pts[None, :] + dy[:, None]) <= 0.3).any(axis=1)
        exact = steep | ~(np.float32(hi) - np.float32(lo) <= np.float32(2) * HALF_RANGE)
        if curvature_gate is not None:
            exact |= np.abs(e[:, 0] - 2 * e[:, 1] + e[:, 2]) / h**2 * (hi - lo) ** 2 / 8 > curvature_gate
        S, E0 = 1.0 + slope, ebm + dm
        e0, e1 = E0 + S * (lo - ebm), E0 + S * (hi - ebm)
        i0 = np.clip(np.trunc(np.clip((e0 - x[0]) * z[0], -1.0, 2.0e9)).astype(int), 0, n - 2)
        w0, w1 = (e0 - x[i0]) * z[i0], (e1 - x[i0]) * z[i0]
        ok = (S > 0.5) & (e0 <= e1) & (w0 >= 1e-4)
        one = ok & (w1 <= 1 - 1e-4)
        up = np.minimum(i0 + 1, n - 2)
        two = ok & ~one & (i0 + 1 <= n - 2) & ((e1 - x[up]) * z[up] <= 1 - 1e-4)
        code = np.where(exact, EXACT, np.where(curved, CURVED, np.where(one, LIN, np.where(two, KINK, SAMPLE))))
        out.append(code)
    return np.stack(out)


# ---- the cases ----


def _disk(D, radius_deg, seed):
    rng = np.random.default_rng(seed)
    r, p = np.radians(radius_deg) * np.sqrt(rng.uniform(0, 1, D)), rng.uniform(0, 2 * np.pi, D)
    off = np.stack([r * np.cos(p), r * np.sin(p)], axis=1)
    off[0] = 0.0
    return off.astype(np.float32)


def _rings(D, radii_deg):
    """The boresight and D - 1 detectors spread over rings of the given radii."""
    k = np.arange(D - 1)
    r = np.radians(np.asarray(radii_deg, float))[k % len(radii_deg)]
    p = 2 * np.pi * (k // len(radii_deg)) / max(1, -(-(D - 1) // len(radii_deg))) + 0.3
    return np.concatenate([[[0.0, 0.0]], np.stack([r * np.cos(p), r * np.sin(p)], axis=1)]).astype(np.float32)


def _sinus(T, centre_deg, amp_deg, period=1900.0):
    return np.radians(centre_deg + amp_deg * np.sin(2 * np.pi * np.arange(T) / period))


def _sweep(T, centre_deg, per_tile):
    """A linear slew of per_tile rad every 1024 samples, centred on centre_deg."""
    s = np.arange(T)
    return np.radians(centre_deg) + per_tile * (s - 0.5 * (T - 1)) / (TILE - 1)


def _gate_track(T, centre_deg, target):
    """A sinusoid whose largest inner-sample deviation from the chord is target rad."""
    shape = np.sin(2 * np.pi * np.arange(T) / 512.0)
    unit = chord_deviation(shape.astype(np.float32)).max()
    return np.radians(centre_deg) + (target / unit) * shape


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    contains: tuple      # (table kind, form) pairs the case must show
    off: np.ndarray      # [D, 2] float32
    bore_el: np.ndarray  # [T] float32
    axis_deg: tuple = (20.0, 90.0)
    pad: int = 0         # floats a row is padded by on the device (3: the scalar load and store path)

    @property
    def shape(self):
        return len(self.off), len(self.bore_el)

    @property
    def band(self):
        return (np.arange(len(self.off)) % 2).astype(np.int32)

    @functools.lru_cache(maxsize=None)
    def table(self, kind):
        axis, values = table(kind, *self.axis_deg)
        axis.setflags(write=False)
        values.setflags(write=False)
        return axis, values

    @functools.cached_property
    def el(self):
        e = el_exact(self.off[:, 0], self.off[:, 1], self.bore_el)
        e.setflags(write=False)
        return e

    @functools.cached_property
    def delta_chain(self):
        """max |float32 chain - el_exact| of oracle.hotpath.broadcast over the case's inputs"""
        from oracle import hotpath

        _, el32 = hotpath.broadcast(self.off, np.zeros(len(self.bore_el), np.float32), self.bore_el)
        return float(np.abs(el32.astype(np.float64) - self.el).max())

    @functools.cached_property
    def curved_tiles(self):
        return np.array([c for *_, c in tile_ranges(self.bore_el)])

    @functools.cached_property
    def chord_ok(self):
        """[T]: the samples of the tiles below the gate of KrjSamples::curved"""
        return ~np.repeat(self.curved_tiles, TILE)[: len(self.bore_el)]

    @functools.cached_property
    def chord(self):
        """[T]: the inner samples' deviation from the chord in the tiles below the gate of KrjSamples::curved (there the
        chord form may be taken), zero elsewhere"""
        return np.where(self.chord_ok, chord_deviation(self.bore_el), 0.0)

    @functools.cached_property
    def b_el(self):
        """[1, T]: 1e-6 rad + delta_chain + the chord deviation of the sample"""
        return (GRANT + self.delta_chain + self.chord)[None, :]

    @functools.lru_cache(maxsize=None)
    def den(self, kind):
        """The reference [D, T] of the case on one table kind, every row on its band."""
        axis, values = self.table(kind)
        d = np.stack([den_exact(axis, values[b], self.el[r]) for r, b in enumerate(self.band)])
        d.setflags(write=False)
        return d

    @functools.lru_cache(maxsize=None)
    def tol(self, kind):
        axis, values = self.table(kind)
        t = np.stack([tol(axis, values[b], self.el[r : r + 1], self.b_el, self.chord_ok)[0] for r, b in enumerate(self.band)])
        t.setflags(write=False)
        return t

    @functools.lru_cache(maxsize=None)
    def exempt(self, kind):
        return near_an_end(self.table(kind)[0], self.el, self.b_el)

    @functools.lru_cache(maxsize=None)
    def straddling(self, kind):
        """[D, T] bool: the samples of the four-sample groups with a straddle allowance."""
        axis, values = self.table(kind)
        return np.stack([np.where(self.chord_ok, straddle(axis, values[b], self.el[r : r + 1])[0], 0.0) for r, b in enumerate(self.band)]) > 0

    @functools.lru_cache(maxsize=None)
    def straddle_share(self, kind):
        """Share of the four-sample groups with a straddle allowance."""
        return float(groups_of(self.straddling(kind))[..., 0].mean())

    @functools.lru_cache(maxsize=None)
    def forms(self, kind, curvature_gate=None):
        return forms(self.off, self.bore_el, self.table(kind)[0], curvature_gate)

    def form_of_samples(self, kind, curvature_gate=None):
        """[D, T] form codes."""
        return np.repeat(self.forms(kind, curvature_gate).T, TILE, axis=1)[:, : len(self.bore_el)]


D0, T0 = 37, 3 * TILE + 5  # a ragged last group of rows (37 = 2 x 16 + 5) and a ragged last tile


def _case(name, contains, off, el, **kw):
    off, el = np.ascontiguousarray(off, np.float32), np.ascontiguousarray(el, np.float32)
    off.setflags(write=False)
    el.setflags(write=False)
    return Case(name, tuple(contains), off, el, **kw)


def track(name, T=T0):
    """The boresight elevation tracks that the writers' tests take at their own length."""
    if name.startswith("sweep"):
        _, centre, per = name.split("_")
        return _sweep(T, float(centre), {"under": 0.039, "over": 0.041}[per])
    if name == "steep":
        return np.radians(np.linspace(70.0, 76.0, T))
    if name == "curved":  # a daisy of 0.1 deg at 0.8 deg/s sampled at 20 Hz
        return np.radians(55.0 + 0.1 * np.sin(8.0 * np.arange(T) / 20.0))
    if name == "off_low":
        return _sinus(T, 60.2, 0.3)
    if name == "off_high":
        return _sinus(T, 61.5, 0.3)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def cases():
    disk = _disk(D0, 0.5, 1)
    rings = _rings(D0, (0.25, 1.0, 1.41))
    out = [
        _case("lin", [("zigzag", "lin"), ("ramp3", "lin")], disk, _sinus(T0, 55.0, 0.3)),
        # node 15 of the axis: 20 + 15 x 2.1875
        _case("kink", [("zigzag", "kink")], disk, _sinus(T0, 20.0 + 15 * CELL_DEG, 0.3)),
        _case("descending", [("zigzag", "lin"), ("zigzag", "kink")], disk, _sinus(T0, 55.0, 0.3)[::-1]),
    ]
    for centre in (50, 60, 68):
        out.append(_case(f"sweep_{centre}_under", [("zigzag", "kink"), ("ramp200", "sample")], rings, track(f"sweep_{centre}_under")))
        out.append(_case(f"sweep_{centre}_over", [("zigzag", "exact")], rings, track(f"sweep_{centre}_over")))
    slew = np.concatenate([_sinus(TILE, 25.0, 0.2), np.radians(np.linspace(25.0, 80.0, TILE)), _sinus(TILE + 5, 80.0, 0.2)])
    gate = {k: _gate_track(T0, 55.0, v) for k, v in (("under", 0.85e-6), ("over", 1.15e-6))}
    out += [
        _case("steep", [("zigzag", "exact"), ("zigzag", "lin")], disk, track("steep")),
        _case("zenith", [("zigzag", "exact")], _disk(D0, 0.2, 2), np.radians(np.linspace(84.0, 89.5, T0))),
        _case("slew", [("zigzag", "exact"), ("zigzag", "lin")], rings, slew),
        _case("curved", [("zigzag", "curved")], disk, track("curved")),
        _case("curved_under", [("zigzag", "lin"), ("zigzag", "kink")], disk, gate["under"]),
        _case("curved_over", [("zigzag", "curved")], disk, gate["over"]),
        _case("off_low", [("zigzag", "sample")], disk, track("off_low"), axis_deg=(60.0, 90.0)),
        _case("off_high", [("zigzag", "sample")], disk, track("off_high"), axis_deg=(20.0, 62.0)),
        # the boresight passes 90.1 deg; no detector does (asin folds at the zenith): no NaN anywhere
        _case("off_zenith", [("zigzag", "exact")], _disk(D0, 0.2, 3), np.radians(np.linspace(89.0, 90.6, T0))),
        # tile 0 linear, tile 1 a slew past the model's range, tile 2 off the axis' high end
        _case("tiles", [("zigzag", "lin"), ("zigzag", "exact"), ("zigzag", "sample")], disk,
              np.concatenate([_sinus(TILE, 56.0, 0.2), np.radians(np.linspace(56.0, 59.0, TILE)), np.radians(np.linspace(61.2, 62.6, TILE + 5))]),
              axis_deg=(20.0, 62.0)),
    ]
    wide = _rings(D0, (3.0, 5.0, 8.0, 18.0))
    for centre in (45, 60):
        out.append(_case(f"wide_{centre}", [], wide, _sinus(T0, float(centre), 0.3)))
    for D in (1, 17):
        for T in (1, 3, 1023, 1025):
            out.append(_case(f"ragged_{D}_{T}", [], _disk(17, 0.5, 4)[17 - D :], _sinus(T0, 55.0, 0.3)[:T], pad=3))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)
