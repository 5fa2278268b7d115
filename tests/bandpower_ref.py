"""float64 numpy restatement of ``mrx_map_band_powers`` (include/mrx.h): the binned sums behind the
TT, EE, BB, TE, TB, EB band powers of two maps, from their half-plane modes.  Nothing here runs on a GPU.

``a1``, ``a2``: [3, ny, nx/2 + 1] complex128, the modes of T, Q, U in numpy.fft.rfft2's layout; ``res`` the pixel size
in radians; ``edges`` [n_bins + 1] ascending.  Per cell, fx = 0 .. nx/2 and fy signed as numpy.fft.fftfreq orders it:

    k = 2 pi (fx / (nx res), fy / (ny res)),  l2 = kx kx + ky ky,  c = (kx kx - ky ky) / l2,  s = 2 kx ky / l2
    E = Q c + U s,  B = -Q s + U c,  XY = (Re(a1_X conj a2_Y) + Re(a1_Y conj a2_X)) / 2,  w = 1 where fx = 0, else 2

dropped: k = 0, fx = nx/2, |fy| = ny/2, l outside [edges[0], edges[-1]); bin b holds edges[b]^2 <= l2 < edges[b+1]^2."""

from __future__ import annotations

import numpy as np

COLUMNS = ("TT", "EE", "BB", "TE", "TB", "EB")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # indices into (T, E, B)


def cells(ny, nx, res, edges):
    """Per cell of the half plane [ny, nx/2 + 1]: (l2, c, s, w, bin); bin = -1 where the cell is dropped."""
    edges = np.asarray(edges, np.float64)
    fy = np.where(np.arange(ny) < ny // 2, np.arange(ny), np.arange(ny) - ny).astype(np.float64)[:, None]
    fx = np.arange(nx // 2 + 1, dtype=np.float64)[None, :]
    kx = 2 * np.pi * (fx / (nx * res))
    ky = 2 * np.pi * (fy / (ny * res))
    l2 = kx * kx + ky * ky
    safe = np.where(l2 > 0, l2, 1.0)
    c = (kx * kx - ky * ky) / safe
    s = (2.0 * kx * ky) / safe
    w = np.where(fx == 0, 1.0, 2.0) + 0 * fy
    e2 = edges * edges
    b = np.full(l2.shape, -1, np.int64)
    for i in range(len(edges) - 1):  # plain masks, bin by bin
        b[(l2 >= e2[i]) & (l2 < e2[i + 1])] = i
    b[l2 == 0] = -1
    b[ny // 2, :] = -1
    b[:, nx // 2] = -1
    return l2, c, s, w, b


def teb(a, c, s):
    """(T, E, B) [ny, nx/2 + 1] of the modes ``a`` [3, ...] of T, Q, U."""
    return a[0], a[1] * c + a[2] * s, -a[1] * s + a[2] * c


def sums(a1, a2, res, edges):
    """(sums [n_bins, 8], scale [n_bins, 6]): per bin sum w, sum w l, sum w XY for TT, EE, BB, TE, TB, EB -- and, per
    bin and power column, sum w (|a1_X| |a2_Y| + |a1_Y| |a2_X|) / 2 with |E| and |B| taken as |Q| + |U|: the size of
    the terms before any of them cancel (B of a pure-E map is all cancellation), the scale of the tolerances."""
    a1 = np.asarray(a1, np.complex128)
    a2 = np.asarray(a2, np.complex128)
    _, ny, nxh = a1.shape
    nx = 2 * (nxh - 1)
    l2, c, s, w, b = cells(ny, nx, res, edges)
    m1, m2 = teb(a1, c, s), teb(a2, c, s)
    g1 = (np.abs(a1[0]), np.abs(a1[1]) + np.abs(a1[2]), np.abs(a1[1]) + np.abs(a1[2]))
    g2 = (np.abs(a2[0]), np.abs(a2[1]) + np.abs(a2[2]), np.abs(a2[1]) + np.abs(a2[2]))
    n_bins = len(edges) - 1
    out, scale = np.zeros((n_bins, 8)), np.zeros((n_bins, 6))
    ell = np.sqrt(l2)
    for i in range(n_bins):
        sel = b == i
        ws = w[sel]
        out[i, 0] = ws.sum()
        out[i, 1] = (ws * ell[sel]).sum()
        for j, (x, y) in enumerate(PAIRS):
            xy = 0.5 * ((m1[x][sel] * np.conj(m2[y][sel])).real + (m1[y][sel] * np.conj(m2[x][sel])).real)
            out[i, 2 + j] = (ws * xy).sum()
            scale[i, j] = (ws * 0.5 * (g1[x][sel] * g2[y][sel] + g1[y][sel] * g2[x][sel])).sum()
    return out, scale


def modes(tqu, window, res):
    """rfft2((tqu - the window-weighted mean of T alone) * window) / (ny nx) in numpy float64: what
    ``maria_amd.bandpowers.modes`` computes on the device.  NaN pixels count as zero window."""
    tqu = np.array(tqu, np.float64)
    if tqu.shape[0] == 1:
        tqu = np.concatenate([tqu, np.zeros((2,) + tqu.shape[1:])])
    ny, nx = tqu.shape[-2:]
    win = np.ones((ny, nx)) if window is None else np.array(window, np.float64)
    bad = ~np.isfinite(tqu).all(axis=0) | ~np.isfinite(win)
    win = np.where(bad, 0.0, win)
    tqu = np.where(bad[None], 0.0, tqu)
    tqu[0] -= (tqu[0] * win).sum() / win.sum()
    return np.fft.rfft2(tqu * win[None], axes=(-2, -1)) / (ny * nx), win


def band_powers(sums_, ny, nx, res, w1, w2=None):
    """(ell [n_bins], cl [n_bins, 6], n_modes [n_bins]) from the sums: C_b = Lx Ly sum w XY / (sum w <W1 W2>)."""
    w2 = w1 if w2 is None else w2
    area = (ny * res) * (nx * res)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums_[:, 1] / sums_[:, 0], area * sums_[:, 2:] / (sums_[:, :1] * np.mean(w1 * w2)), sums_[:, 0]


def expected(cl, ny, nx, res, edges):
    """[n_bins, 4] (TT, EE, BB, TE): the mean of the input table ``cl`` [n_ell, 4] over the very cells of each bin, with
    the cells' weights, C(l) interpolated linearly between the integer rows (zero beyond the last); NaN for an empty bin."""
    cl = np.asarray(cl, np.float64)
    l2, _, _, w, b = cells(ny, nx, res, edges)
    ell = np.sqrt(l2)
    n = len(cl)
    l0 = np.minimum(ell.astype(np.int64), n - 2)
    val = cl[l0] + (ell - l0)[..., None] * (cl[np.minimum(l0 + 1, n - 1)] - cl[l0])
    val[ell > n - 1] = 0.0
    out = np.full((len(edges) - 1, 4), np.nan)
    for i in range(len(edges) - 1):
        sel = b == i
        if sel.any():
            out[i] = (w[sel][:, None] * val[sel]).sum(axis=0) / w[sel].sum()
    return out
