"""The pixel of every sample against an exact pointing.  Plain numpy, no torch.

Steps 1-3 of the map operators (mrx_map_pointing.h: the detector's az/el, the frame rotation, the offsets from the map
centre) evaluated without rounding between the steps, on the numbers the device receives; the float32 restatement of the same
chain through the oracle; the radius eps that separates the two plus the bound the device forms are held to against the
restatement; and, per axis, the set of pixels a sample may take: the nearest nodes of the points within eps of the exact
offset.  tests/test_host_pointing_ref.py checks this module on the CPU, tests/test_gpu_map_pixels.py the kernels against it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

DEVICE_BOUND = 6e-7  # rad: what both device forms are held to against the float32 restatement (tests/test_gpu_map.py)
EPS_MAX = 1.2e-6     # rad: a case whose eps is larger than this is not sharp enough to be a test
AMBIGUOUS_MAX = 0.25  # the largest share of samples whose accepted set has more than one pixel
R2_FAR = 0.01        # sin^2 of the offset from which sample_offsets takes the function instead of the series
WAVE = 64


def exact_offsets(off, az, el, transform, centre, dtype=np.longdouble):
    """(xi, eta) offsets [D, T, 2] float64 of every detector sample from the map centre: steps 1-3 in ``dtype`` with no
    rounding between them.  off [D, 2] (dx, dy) and az, el [T] are taken as the float32 numbers the device receives,
    transform [T, 3, 3] float64 or None, centre (cphi, ctheta) with cphi rounded to float32 (as jax demotes it and as the
    kernel's g.cphi holds it).  pi / 2 is ``dtype``'s, not the float32 constant of the chain."""
    ft = dtype
    half_pi = np.arccos(ft(0))
    dx = np.asarray(off, np.float32)[:, 0].astype(ft)[:, None]
    dy = np.asarray(off, np.float32)[:, 1].astype(ft)[:, None]
    az = np.asarray(az, np.float32).astype(ft)[None, :]
    el = np.asarray(el, np.float32).astype(ft)[None, :]
    # 1. detector az/el (transforms.py:10-29): (sin r cos p + i cos r) exp(i (el - pi/2)), p = atan2(-dx, -dy)
    r = np.sqrt(dx * dx + dy * dy)
    p = np.arctan2(-dx, -dy)
    a_re, a_im = np.sin(r) * np.cos(p), np.cos(r)
    b_re, b_im = np.cos(el - half_pi), np.sin(el - half_pi)
    re, im = a_re * b_re - a_im * b_im, a_re * b_im + a_im * b_re
    phi = np.arctan2(np.sin(r) * np.sin(p), re) + az
    theta = np.arcsin(im)
    # 2. frame rotation (coordinates.py:220-230): the unit vector times the sample's 3 x 3, back to angles
    if transform is not None:
        M = np.asarray(transform, np.float64).astype(ft)  # [T, 3, 3]
        v = np.stack([np.cos(phi) * np.cos(theta), np.sin(phi) * np.cos(theta), np.sin(theta)], axis=-1)  # [D, T, 3]
        w = (v[..., :, None] * M[None]).sum(axis=-2)
        phi = np.mod(np.arctan2(w[..., 1], w[..., 0]), 4 * half_pi)
        theta = np.arcsin(w[..., 2] / np.sqrt((w * w).sum(axis=-1)))
    # 3. offsets from the map centre (transforms.py:36-53)
    cphi, ctheta = ft(np.float32(centre[0])), ft(centre[1])
    dphi = phi - cphi
    rot_re, rot_im = np.cos(half_pi - ctheta), np.sin(half_pi - ctheta)
    proj_re = np.cos(dphi) * np.cos(theta) * rot_re - np.sin(theta) * rot_im
    dz_re, dz_im = np.sin(dphi) * np.cos(theta), proj_re
    rr = np.sqrt(dz_re * dz_re + dz_im * dz_im)
    f = np.arcsin(rr) / np.where(rr > 0, rr, ft(1))
    return np.stack([-dz_re * f, -dz_im * f], axis=-1).astype(np.float64)


def oracle_offsets(off, az, el, transform, centre):
    """The same offsets through the float32 restatement of the reference chain (oracle.hotpath.broadcast,
    oracle.mapsample.frame_angles and phi_theta_to_offsets), [D, T, 2] float64 of float32 numbers."""
    from oracle import hotpath, mapsample

    az_d, el_d = hotpath.broadcast(off, np.asarray(az, np.float32), np.asarray(el, np.float32))
    phi, theta = mapsample.frame_angles(az_d, el_d, transform)
    return mapsample.phi_theta_to_offsets(phi, theta, centre[0], centre[1]).astype(np.float64)


def epsilon(off, az, el, transform, centre, exact=None):
    """max |oracle_offsets - exact_offsets| + 6e-7 rad: nothing in it is measured on the device."""
    exact = exact_offsets(off, az, el, transform, centre) if exact is None else exact
    return float(np.abs(oracle_offsets(off, az, el, transform, centre) - exact).max()) + DEVICE_BOUND


def accepted(x, first, step, n, eps):
    """(lo, hi) integer arrays: the nodes of the axis first + i step, i = 0 .. n - 1 (step of either sign), that are the
    nearest node of some point of [x - eps, x + eps]; a point beyond an end of the axis takes the end node."""
    x = np.asarray(x, np.float64)
    a = np.floor((x - eps - first) / step + 0.5)
    b = np.floor((x + eps - first) / step + 0.5)
    lo = np.clip(np.minimum(a, b), 0, n - 1).astype(np.int64)
    hi = np.clip(np.maximum(a, b), 0, n - 1).astype(np.int64)
    return lo, hi


def ambiguous_share(lo_eta, hi_eta, lo_xi, hi_xi):
    """Share of the samples whose accepted set holds more than one pixel."""
    return float(((hi_eta > lo_eta) | (hi_xi > lo_xi)).mean())


def check_pixels(rows, cols, lo_eta, hi_eta, lo_xi, hi_xi):
    """Boolean array: the sample's (row, column) lies in its accepted set.  Every sample is judged; there is no allowance."""
    rows, cols = np.asarray(rows), np.asarray(cols)
    return (rows >= lo_eta) & (rows <= hi_eta) & (cols >= lo_xi) & (cols <= hi_xi)


def clip_to_axis(x, first, step, n):
    """x clipped to the axis' two end nodes: what a ramp map returns for a sample beyond them."""
    last = first + (n - 1) * step
    return np.clip(x, min(first, last), max(first, last))


# ---- the cases ----


def scan(D=37, T=3001, fov_deg=0.4):
    """tests/test_gpu_map.py::_scan: a daisy at az ~ 0.78, el ~ 1.05 at 50 Hz, a hexagonal focal plane rolled by 11 degrees;
    D and T are no multiples of the tile's 16 rows and 1024 samples."""
    from test_gpu_map import _scan

    return _scan(D=D, T=T, fov_deg=fov_deg)


@dataclass(frozen=True)
class Axis:
    first: float
    step: float
    n: int

    @property
    def nodes(self):
        return self.first + self.step * np.arange(self.n)

    @property
    def c_frac(self):
        """The fraction of -first / step: where zero lies between two nodes (mrx_map_pointing.h, Axis::c_frac)."""
        c = -self.first / self.step
        return c - np.floor(c)


@dataclass(frozen=True)
class Case:
    name: str
    fov_deg: float
    frame: str     # "az/el" or "sky"
    pixel: float   # rad

    @functools.cached_property
    def inputs(self):
        """(t, az, el, off, transform, centre)"""
        from test_gpu_map import _centre, _sky_rotation

        t, az, el, off = scan(fov_deg=self.fov_deg)
        transform = _sky_rotation(t) if self.frame == "sky" else None
        return t, az, el, off, transform, _centre(az, el, transform)

    @property
    def pointing(self):
        """what exact_offsets, oracle_offsets and epsilon take"""
        t, az, el, off, transform, centre = self.inputs
        return off, az, el, transform, centre

    @functools.cached_property
    def exact(self):
        x = exact_offsets(*self.pointing)
        x.setflags(write=False)
        return x

    @functools.cached_property
    def e_oracle(self):
        return float(np.abs(oracle_offsets(*self.pointing) - self.exact).max())

    @property
    def eps(self):
        return self.e_oracle + DEVICE_BOUND

    def _axis(self, comp, shift, descending):
        # 0.9 of the largest |offset|: some samples fall off either end; the first node moved by `shift` of a pixel off the
        # symmetric place, so that zero is on no node and on no midpoint
        half = 0.9 * float(np.abs(self.exact[..., comp]).max())
        n = int(np.floor(2 * half / self.pixel)) + 1
        first = (-0.5 * (n - 1) + shift) * self.pixel
        return Axis(-first, -self.pixel, n) if descending else Axis(first, self.pixel, n)

    @functools.cached_property
    def eta(self):
        return self._axis(1, -0.37, True)  # descending: first node at (+(n - 1) / 2 + 0.37) pixel

    @functools.cached_property
    def xi(self):
        return self._axis(0, 0.21, False)

    @functools.cached_property
    def sets(self):
        """(lo_eta, hi_eta, lo_xi, hi_xi), each [D, T]"""
        out = (*accepted(self.exact[..., 1], self.eta.first, self.eta.step, self.eta.n, self.eps),
               *accepted(self.exact[..., 0], self.xi.first, self.xi.step, self.xi.n, self.eps))
        for a in out:
            a.setflags(write=False)
        return out

    @functools.cached_property
    def clipped(self):
        """The exact offsets clipped to the axes' end nodes, [D, T, 2] (xi, eta)."""
        x = np.stack([clip_to_axis(self.exact[..., 0], self.xi.first, self.xi.step, self.xi.n),
                      clip_to_axis(self.exact[..., 1], self.eta.first, self.eta.step, self.eta.n)], axis=-1)
        x.setflags(write=False)
        return x

    def off_map_shares(self):
        """Share of the samples more than half a pixel beyond each of the four ends: (eta first, eta last, xi first, xi
        last)."""
        out = []
        for comp, ax in ((1, self.eta), (0, self.xi)):
            u = (self.exact[..., comp] - ax.first) / ax.step
            out += [float((u < -0.5).mean()), float((u > ax.n - 0.5).mean())]
        return tuple(out)

    def mixed_wave(self):
        """(detector, first sample) of 64 consecutive samples of one row, starting at a multiple of 64, that hold sin^2 of
        the offset on both sides of 0.01 (by more than float32 rounding): both sides of sample_offsets' ballot in one
        wave.  None if there is none."""
        r2 = np.sin(np.hypot(self.exact[..., 0], self.exact[..., 1])) ** 2
        T = r2.shape[1] // WAVE * WAVE
        w = r2[:, :T].reshape(r2.shape[0], -1, WAVE)
        both = (w.min(axis=-1) < R2_FAR - 1e-5) & (w.max(axis=-1) > R2_FAR + 1e-5)
        hit = np.argwhere(both)
        return None if len(hit) == 0 else (int(hit[0, 0]), int(hit[0, 1]) * WAVE)


@functools.lru_cache(maxsize=None)
def cases():
    """The four cases: a coarse control, two fine grids (pixel indices in the hundreds and past a
    thousand, in both frames) and a wide field whose offsets pass 0.1 rad."""
    return (Case("A", 2.0, "az/el", 5e-4), Case("B", 0.4, "sky", 3e-5), Case("C", 0.4, "az/el", 2e-5), Case("W", 12.0, "sky", 1e-4))
