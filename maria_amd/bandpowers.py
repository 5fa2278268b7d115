"""Band powers from maps: binned TT, EE, BB, TE, TB, EB of one map or of a pair, on the device.

The last step of the loop ``CMB.generate`` -> ``Simulation(cmb=...)`` -> TOD cleaning -> ``MaximumLikelihoodMapper``:
a spectrum measured from a map, to set against the C_ell that went in (``expected``), and a filter's transfer function
(``transfer_function``).  The transform is ``torch.fft.rfft2`` in float64 on the device (``modes``); the rotation of
Q / U into E / B, the binning and the sums are ``mrx_map_band_powers`` (csrc/mrx_spectrum.hip): float64, no atomics, the
same bits on every call.

Conventions are those of ``maria_amd.cmb``: a map is [3, ny, nx] (T, Q, U; rows y = eta ascending, columns x = xi), ``res``
the pixel size in radians, a spectrum ``cl`` [n_ell, 4] in K^2 (TT, EE, BB, TE; row = integer ell)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

COLUMNS = ("TT", "EE", "BB", "TE", "TB", "EB")
_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # a column's two fields out of (T, E, B)
MAX_BINS = 1024


def bin_edges(first, width, ell_max):
    """Uniform edges first, first + width, ... up to and including the last one <= ``ell_max``."""
    if not (first >= 0 and width > 0 and ell_max >= first + width):
        raise ValueError("need first >= 0, width > 0 and ell_max >= first + width")
    return check_edges(first + width * np.arange(int(np.floor((ell_max - first) / width + 1e-9)) + 1))


def check_edges(edges):
    """Caller-given edges as the float64 array the kernel takes: finite, >= 0, strictly ascending, 1 .. 1024 bins."""
    edges = np.ascontiguousarray(edges, np.float64)
    if edges.ndim != 1 or not 2 <= len(edges) <= MAX_BINS + 1:
        raise ValueError(f"edges must be a 1-D array of 2 .. {MAX_BINS + 1} values")
    if not np.isfinite(edges).all() or edges[0] < 0 or not (np.diff(edges) > 0).all():
        raise ValueError("edges must be finite, not negative and strictly ascending")
    return edges


def taper(ny, nx, frac):
    """A separable cosine taper [ny, nx] float64: along each axis of n pixels the first and last m = frac n / 2 pixels
    rise as sin^2(pi (i + 1/2) / (2 m)) (the Hann edge, sampled at pixel centres), the rest is 1; frac in [0, 1]."""
    if not 0 <= frac <= 1:
        raise ValueError("frac must be in [0, 1]")

    def axis(n):
        m = 0.5 * frac * n
        d = np.minimum(np.arange(n) + 0.5, n - 0.5 - np.arange(n))  # distance from the nearer edge, in pixels
        return np.where(d < m, np.sin(0.5 * np.pi * d / m) ** 2, 1.0) if m > 0 else np.ones(n)

    return axis(ny)[:, None] * axis(nx)[None, :]


def weight_mask(weight, floor=0.1):
    """The binary mask of ``window_from_weight``: 1.0 where weight > floor x the median of the positive weights (NaN
    and unhit pixels: 0.0)."""
    w = np.asarray(weight, np.float64)
    if w.ndim != 2:
        raise ValueError("weight must be [ny, nx]")
    pos = w[np.isfinite(w) & (w > 0)]
    if pos.size == 0:
        raise ValueError("no pixel has a positive weight")
    return (np.nan_to_num(w, nan=0.0) > floor * np.median(pos)).astype(np.float64)


def window_from_weight(weight, sigma_px, floor=0.1, device="cuda:0", ctx=None):
    """A smooth window [ny, nx] float64 that vanishes at the edge of a map's coverage, from its ``weight`` [ny, nx]:
    the mask ``weight_mask(weight, floor)`` smoothed by a Gaussian of ``sigma_px`` pixels (``mrx_gauss_smooth2d``, the
    stencil of ``ProjectionMap.smooth``), set to zero where that is < 0.99 -- which moves the edge about 2.3 sigma
    inwards -- and smoothed again.  The map's own border counts as an edge of the coverage: the mask is smoothed inside
    a frame of zeros one stencil radius wide (the stencil reflects at the border of what it is given, and hits that
    reach the border would otherwise keep the window at 1 there), and the frame is cut off again."""
    from ._lib import Context, ptr

    if not sigma_px > 0:
        raise ValueError("sigma_px must be positive")
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    ctx = ctx or Context(dev.index or 0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    pad = int(4.0 * sigma_px + 0.5) + 1  # the stencil's radius and a pixel
    m = torch.nn.functional.pad(torch.as_tensor(weight_mask(weight, floor).astype(np.float32)).to(dev), (pad, pad, pad, pad)).contiguous()
    ny, nx = m.shape
    tmp = torch.empty_like(m)
    ctx.call("mrx_gauss_smooth2d", ptr(m), ptr(m), ptr(tmp), ny, nx, float(sigma_px), float(sigma_px), 4.0)
    m = torch.where(m < 0.99, torch.zeros_like(m), m)
    ctx.call("mrx_gauss_smooth2d", ptr(m), ptr(m), ptr(tmp), ny, nx, float(sigma_px), float(sigma_px), 4.0)
    return m[pad:-pad, pad:-pad].clamp(0.0, 1.0).cpu().numpy().astype(np.float64)


@dataclass
class Modes:
    """``modes``' result: ``a`` [3, ny, nx/2 + 1] complex128 on the device, the ``window`` [ny, nx] float64 as used
    (zero on NaN pixels), ``res``."""

    a: torch.Tensor
    window: torch.Tensor
    res: float

    @property
    def shape(self):
        return tuple(self.window.shape)


def modes(tqu, window=None, res=None, device="cuda:0"):
    """The half-plane modes of a map: ``rfft2((tqu - the window-weighted mean of T alone) * window) / (ny nx)`` in float64
    on the device.  ``tqu``: [3, ny, nx], or I alone as [1, ny, nx] (Q = U = 0), an array or a tensor; ``window``
    [ny, nx] or None (ones).  A pixel that is NaN in any field (a map's unhit pixels) or in the window counts as zero
    window.  ny and nx must be even and at least 8."""
    if res is None or not res > 0:
        raise ValueError("res (radians a pixel) must be positive")
    dev = torch.device(device)
    t = (tqu if isinstance(tqu, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(tqu))).to(dev, torch.float64)
    if t.ndim != 3 or t.shape[0] not in (1, 3):
        raise ValueError("a map must be [3, ny, nx] (T, Q, U) or [1, ny, nx] (I alone)")
    ny, nx = t.shape[-2:]
    if ny < 8 or nx < 8 or ny % 2 or nx % 2:
        raise ValueError(f"map sides must be even and at least 8 (got {ny} x {nx})")
    if t.shape[0] == 1:
        t = torch.cat([t, torch.zeros((2, ny, nx), dtype=torch.float64, device=dev)])
    if window is None:
        win = torch.ones((ny, nx), dtype=torch.float64, device=dev)
    else:
        win = (window if isinstance(window, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(window))).to(dev, torch.float64)
        if tuple(win.shape) != (ny, nx):
            raise ValueError(f"window of shape {tuple(win.shape)} does not match the map's {(ny, nx)}")
    bad = ~torch.isfinite(t).all(dim=0) | ~torch.isfinite(win)
    win = torch.where(bad, torch.zeros_like(win), win)
    t = torch.where(bad[None], torch.zeros_like(t), t)
    total = win.sum()
    if not float(total) > 0:
        raise ValueError("the window is zero everywhere")
    t[0] -= (t[0] * win).sum() / total
    a = torch.fft.rfft2(t * win[None], dim=(-2, -1)) / (ny * nx)
    return Modes(a.contiguous(), win, float(res))


def binned_sums(m1, m2, edges, ctx=None):
    """``mrx_map_band_powers`` on two ``Modes`` (``m2 is m1``: the auto spectra) -> [n_bins, 8] float64 on the host:
    sum w, sum w l, then sum w XY for TT, EE, BB, TE, TB, EB."""
    from . import _lib
    from ._lib import Context, ptr

    edges = check_edges(edges)
    if m2.shape != m1.shape or m2.res != m1.res:
        raise ValueError(f"the two maps differ in shape or pixel size: {m1.shape} at {m1.res} and {m2.shape} at {m2.res}")
    dev = m1.a.device
    if m2.a.device != dev:
        raise ValueError("the two maps' modes are on different devices")
    torch.cuda.set_device(dev)
    ctx = ctx or Context(dev.index or 0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    ny, nx = m1.shape
    n_bins = len(edges) - 1
    need = C.c_size_t()
    if _lib.load().mrx_band_power_work_bytes(ny, nx, n_bins, C.byref(need)) != _lib.MRX_OK:
        raise ValueError("mrx_band_power_work_bytes: sides must be even and >= 8, n_bins in 1 .. 1024")
    work = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty((n_bins, 8), dtype=torch.float64, device=dev)
    ctx.call("mrx_map_band_powers", ptr(m1.a), ptr(m2.a), ny, nx, m1.res, edges.ctypes.data_as(C.POINTER(C.c_double)), n_bins,
             ptr(out), ptr(work), need.value)
    return out.cpu().numpy()


def _cells(ny, nx, res, edges):
    """(l, w, bin) of every cell of the half plane on the host, bin = -1 where the kernel drops the cell."""
    fy = np.where(np.arange(ny) < ny // 2, np.arange(ny), np.arange(ny) - ny).astype(np.float64)[:, None]
    fx = np.arange(nx // 2 + 1, dtype=np.float64)[None, :]
    kx, ky = 2 * np.pi * (fx / (nx * res)), 2 * np.pi * (fy / (ny * res))
    l2 = kx * kx + ky * ky
    b = np.searchsorted(edges * edges, l2, side="right") - 1
    b[(b >= len(edges) - 1) | (l2 == 0)] = -1
    b[ny // 2, :] = -1
    b[:, nx // 2] = -1
    return np.sqrt(l2), np.where(fx == 0, 1.0, 2.0) + 0 * fy, b


@dataclass
class BandPowers:
    """Binned spectra.  ``ell`` [n_bins]: sum w l / sum w of each bin's cells; ``edges`` [n_bins + 1]; ``n_modes``
    [n_bins]: sum w, the cells of the full plane in the bin; ``cl`` [n_bins, 6] in the map's units squared (K^2);
    ``columns``; ``sigma`` [n_bins, 6]: Knox's estimate (see ``band_powers``).  Empty bins are NaN with ``n_modes`` 0.
    ``shape`` and ``res`` are the map's: what ``expected`` needs to find each bin's cells again."""

    ell: np.ndarray
    edges: np.ndarray
    n_modes: np.ndarray
    cl: np.ndarray
    sigma: np.ndarray
    shape: tuple
    res: float
    columns: tuple = field(default=COLUMNS)

    def to_dl(self):
        """``(ell, D_ell [n_bins, 6])`` in uK^2: D = ell (ell + 1) C / 2 pi x 1e12 at each bin's ``ell``, as
        ``cmb.to_dl`` defines it for a table."""
        return self.ell, self.cl * (self.ell * (self.ell + 1.0) / (2.0 * np.pi))[:, None] * 1e12


def from_sums(sums, edges, shape, res, w12=1.0, w1122=1.0, beam_fwhm=None, transfer=None):
    """The host half of ``band_powers``: ``BandPowers`` from the kernel's ``sums`` [n_bins, 8], the window moments
    ``w12`` = <W1 W2> and ``w1122`` = <W1^2 W2^2> (means over pixels), the beam and the transfer function."""
    sums = np.asarray(sums, np.float64)
    edges = check_edges(edges)
    n_bins = len(edges) - 1
    if sums.shape != (n_bins, 8):
        raise ValueError(f"sums must be [{n_bins}, 8]")
    ny, nx = shape
    n = sums[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        ell = sums[:, 1] / n
        cl = (ny * res) * (nx * res) * sums[:, 2:] / (n * w12)[:, None]
        if beam_fwhm is not None:
            sigma_beam = float(beam_fwhm) / np.sqrt(8.0 * np.log(2.0))
            cl = cl / np.exp(-ell * (ell + 1.0) * sigma_beam**2)[:, None]
        if transfer is not None:
            tf = np.asarray(transfer, np.float64)
            if tf.shape not in ((n_bins,), (n_bins, 6)):
                raise ValueError(f"transfer must be [{n_bins}] or [{n_bins}, 6]")
            cl = cl / (tf[:, None] if tf.ndim == 1 else tf)
        nu = n * w12**2 / w1122
        sigma = np.stack([np.sqrt((cl[:, x] * cl[:, y] + cl[:, j] ** 2) / nu) for j, (x, y) in enumerate(_PAIRS)], axis=1)
    return BandPowers(ell, edges, n.copy(), cl, sigma, (int(ny), int(nx)), float(res))


def _as_tqu(m, res):
    """([S, ny, nx] array or tensor with rows eta ascending, res in radians, flipped?) of a ProjectionMap or an array."""
    if hasattr(m, "stokes") and hasattr(m, "data"):
        if not np.isclose(abs(m.x_res), abs(m.y_res), rtol=1e-9):
            raise ValueError("band powers need square pixels")
        stokes = m.stokes
        if not set(stokes) <= set("IQU") or ("Q" in stokes) != ("U" in stokes):
            raise ValueError(f"stokes '{stokes}': band powers take I, IQU or QU")
        data = np.asarray(m.data)[:, 0]  # the first channel
        flipped = m.eta[0] > m.eta[-1]   # ProjectionMap's parity: back to the rows E and B are defined on
        if flipped:
            data = data[:, ::-1]
        planes = [data[stokes.index(s)] if s in stokes else np.zeros(data.shape[-2:], data.dtype) for s in ("IQU" if "Q" in stokes else "I")]
        return np.stack(planes), float(abs(m.x_res)), flipped
    if res is None:
        raise ValueError("an array needs res= (radians a pixel)")
    return m, float(res), False


def _as_window(w, flipped):
    if w is None or not flipped:
        return w
    return torch.flip(w, dims=(0,)) if isinstance(w, torch.Tensor) else np.asarray(w)[::-1].copy()


def band_powers(map1, map2=None, window=None, window2=None, edges=None, beam_fwhm=None, transfer=None, res=None,
                device="cuda:0", ctx=None):
    """Binned TT, EE, BB, TE, TB, EB of ``map1``, or the cross spectra of ``map1`` and ``map2`` -> ``BandPowers``.

    This is a PSEUDO-spectrum: the windowed map's modes, binned and divided by the window's mean square.  There is no
    mode-coupling matrix and no E/B purification: a window mixes neighbouring multipoles and leaks E into B.  Calibrate
    that leakage with simulations through ``transfer_function`` and pass the result as ``transfer``.

    A map is a ``ProjectionMap`` (its first channel; Stokes by its ``stokes`` string, "I", "IQU" or "QU"; square
    pixels; rows are put back in ascending eta, and a window's rows follow the map's) or an array / tensor [3, ny, nx]
    or [1, ny, nx] with ``res=`` in radians.  ``window`` [ny, nx] weighs ``map1``, ``window2`` (default ``window``)
    ``map2``; NaN pixels count as zero window.  ``edges``: ``bin_edges(...)`` or any ascending array.

        C_b = Lx Ly sum w XY / (sum w <W1 W2>)          (the sums of ``mrx_map_band_powers``; <> the mean over pixels)

    then divided by exp(-l_b (l_b + 1) sigma_beam^2) for a Gaussian beam of ``beam_fwhm`` radians and by ``transfer``
    [n_bins] or [n_bins, 6].  ``sigma`` is Knox's formula with nu_b = sum w <W1 W2>^2 / <W1^2 W2^2> modes:
    sqrt((C_XX C_YY + C_XY^2) / nu_b), which is C_b sqrt(2 / nu_b) for an auto spectrum."""
    if edges is None:
        raise ValueError("edges are required: bin_edges(first, width, ell_max) or an ascending array")
    edges = check_edges(edges)
    t1, res1, flip1 = _as_tqu(map1, res)
    m1 = modes(t1, _as_window(window, flip1), res1, device=device)
    if map2 is None:
        if window2 is not None:
            raise ValueError("window2 goes with map2")
        m2 = m1
    else:
        t2, res2, flip2 = _as_tqu(map2, res)
        if tuple(t2.shape[-2:]) != m1.shape or not np.isclose(res2, res1, rtol=1e-9):
            raise ValueError(f"the two maps differ in shape or pixel size: {m1.shape} at {res1} and {tuple(t2.shape[-2:])} at {res2}")
        m2 = modes(t2, _as_window(window if window2 is None else window2, flip2), res1, device=device)
    sums = binned_sums(m1, m2, edges, ctx=ctx)
    w12 = m1.window * m2.window
    return from_sums(sums, edges, m1.shape, res1, float(w12.mean()), float((w12 * w12).mean()), beam_fwhm, transfer)


def transfer_function(inputs, outputs, **kw):
    """A filter's transfer function per bin and column [n_bins, 6], to pass as ``transfer=``: the mean over the pairs
    (input map, the map that came out) of the cross power <out x in> over the mean auto power <in x in>.  ``kw`` goes to
    ``band_powers`` (edges, window, res, ...).  NaN where the inputs hold no power (BB of a pure-E sky)."""
    if len(inputs) != len(outputs) or not len(inputs):
        raise ValueError("need as many outputs as inputs, and at least one pair")
    if "transfer" in kw or "beam_fwhm" in kw:
        raise ValueError("the transfer function is measured without transfer= and beam_fwhm=")
    cross = np.mean([band_powers(o, i, **kw).cl for i, o in zip(inputs, outputs)], axis=0)
    auto = np.mean([band_powers(i, **kw).cl for i in inputs], axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(auto != 0, cross / auto, np.nan)


def expected(cl, bp):
    """What ``bp`` should be compared with: the mean of the input table ``cl`` [n_ell, 4] (TT, EE, BB, TE) over the very
    cells of each bin, with the cells' weights, C(l) linear between the integer rows and zero beyond the last ->
    [n_bins, 4]; NaN for an empty bin.  On the host."""
    cl = np.asarray(cl, np.float64)
    if cl.ndim != 2 or cl.shape[1] != 4 or len(cl) < 2:
        raise ValueError("cl must be [n_ell, 4] (TT, EE, BB, TE; row = ell)")
    ell, w, b = _cells(*bp.shape, bp.res, bp.edges)
    n = len(cl)
    l0 = np.minimum(ell.astype(np.int64), n - 2)
    val = cl[l0] + (ell - l0)[..., None] * (cl[np.minimum(l0 + 1, n - 1)] - cl[l0])
    val[ell > n - 1] = 0.0
    out = np.full((len(bp.edges) - 1, 4), np.nan)
    for i in range(len(out)):
        sel = b == i
        if sel.any():
            out[i] = (w[sel][:, None] * val[sel]).sum(axis=0) / w[sel].sum()
    return out
