"""float64 numpy restatement of the CMB patch ``mrx_cmb_generate`` defines (include/mrx.h), and the
estimator the tests read spectra back with.  Nothing here runs on a GPU.

Conventions: a field is [ny, nx] (rows y, columns x), a half spectrum [ny, nx/2 + 1] in numpy.fft.rfft2's layout,
``res`` the pixel size in radians, ``table`` the float32 [n_ell, 4] coefficients of ``maria_amd.cmb.spectrum_table``
(cT, cTE, cE, cB; row = integer ell; carrying 1 / sqrt(Lx Ly))."""

from __future__ import annotations

import numpy as np

TAG = 0x434D4200  # counter word 3 of the CMB draws, | draw index


def wavenumbers(ny, nx, res):
    """(ky [ny, 1], kx [1, nx/2 + 1]) of the half plane, signed as numpy.fft.fftfreq (the Nyquist rows are negative)."""
    ky = 2 * np.pi * np.fft.fftfreq(ny, res)[:, None]
    kx = 2 * np.pi * np.fft.rfftfreq(nx, res)[None, :]
    return ky, kx


def rotation(ny, nx, res):
    """(ell, cos 2 phi, sin 2 phi) [ny, nx/2 + 1], phi = atan2(ky, kx); (1, 0) at k = 0."""
    ky, kx = wavenumbers(ny, nx, res)
    k2 = kx * kx + ky * ky
    safe = np.where(k2 > 0, k2, 1.0)
    return np.sqrt(k2), np.where(k2 > 0, (kx * kx - ky * ky) / safe, 1.0), np.where(k2 > 0, 2 * kx * ky / safe, 0.0)


def nyquist_mask(ny, nx):
    """True on the cells of either Nyquist line of the half plane."""
    m = np.zeros((ny, nx // 2 + 1), bool)
    m[ny // 2, :] = True
    m[:, nx // 2] = True
    return m


def coefficients(table, ell):
    """The four coefficients at ``ell`` (any shape): linear in ell between the integer rows, zero beyond the last."""
    table = np.asarray(table, np.float64)
    n = len(table)
    l0 = np.minimum(ell.astype(np.int64), n - 2)
    w = ell - l0
    out = table[l0] + w[..., None] * (table[np.minimum(l0 + 1, n - 1)] - table[l0])
    out[ell > n - 1] = 0.0
    return np.moveaxis(out, -1, 0)  # [4, ...]


def philox_normals(philox4x32, seed, stream, ny, nx):
    """g [3, ny, nx/2 + 1]: the unit complex normals (E |g|^2 = 1) of every cell, drawn as the kernel draws them --
    counter (kx, iy, stream, TAG | d), words (0, 1) for cell ky = iy, (2, 3) for cell iy + ny/2."""
    half = ny // 2
    words = np.empty((3, nx // 2 + 1, half, 4), np.float64)
    for d in range(3):
        for ix in range(nx // 2 + 1):
            for iy in range(half):
                words[d, ix, iy] = philox4x32(seed, (ix, iy, stream, TAG | d))
    w = words.astype(np.int64)
    g = np.empty((3, ny, nx // 2 + 1), complex)
    for lo, rows in ((0, slice(0, half)), (2, slice(half, ny))):
        u1 = ((w[..., lo] >> 8) + 0.5) / 16777216.0
        u2 = (w[..., lo + 1] >> 8) / 16777216.0
        z = np.sqrt(-2 * np.log(u1)) * np.exp(2j * np.pi * u2) / np.sqrt(2)
        g[:, rows, :] = np.swapaxes(z, 1, 2)
    return g


def numpy_normals(rng, ny, nx):
    """Unit complex normals from a numpy generator instead: the host tests' realisations."""
    shape = (3, ny, nx // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def half_spectra(g, ny, nx, res, table, nyquist=True):
    """a_T, a_Q, a_U [3, ny, nx/2 + 1] from the normals: the correlated draw, the rotation, the Nyquist rule
    (``nyquist=False`` leaves power on the two lines: what the B test must catch), and the symmetrisation of the
    self-mirrored columns, S' = (S[ky] + conj S[-ky]) / sqrt 2 with the self-conjugate cells sqrt 2 Re S."""
    ell, c2, s2 = rotation(ny, nx, res)
    cT, cTE, cE, cB = coefficients(table, ell)
    T = cT * g[0]
    E = cTE * g[0] + cE * g[1]
    B = cB * g[2]
    P = np.stack([T, E * c2 - B * s2, E * s2 + B * c2])
    if nyquist:
        P[:, nyquist_mask(ny, nx)] = 0.0
    half = ny // 2
    for ix in (0, nx // 2):
        col = P[:, :, ix].copy()
        new = col.copy()
        for iy in range(1, half):
            new[:, iy] = (col[:, iy] + np.conj(col[:, ny - iy])) / np.sqrt(2)
            new[:, ny - iy] = np.conj(new[:, iy])
        new[:, 0], new[:, half] = np.sqrt(2) * col[:, 0].real, np.sqrt(2) * col[:, half].real
        P[:, :, ix] = new
    return P


def fields(P, ny, nx):
    """m_X(x_j) = sum_k a_X(k) exp(i k.x_j): T, Q, U [3, ny, nx] float64."""
    return np.fft.irfft2(P, s=(ny, nx), axes=(-2, -1)) * (ny * nx)


def reference_fields(philox4x32, seed, stream, ny, nx, res, table):
    return fields(half_spectra(philox_normals(philox4x32, seed, stream, ny, nx), ny, nx, res, table), ny, nx)


def modes_of(tqu, res):
    """(a_T, a_E, a_B) [ny, nx/2 + 1] read back from whole-domain maps [3, ny, nx] by rfft2."""
    tqu = np.asarray(tqu, np.float64)
    ny, nx = tqu.shape[-2:]
    a = np.fft.rfft2(tqu, axes=(-2, -1)) / (ny * nx)
    _, c2, s2 = rotation(ny, nx, res)
    return a[0], a[1] * c2 + a[2] * s2, -a[1] * s2 + a[2] * c2


def independent_cells(ny, nx):
    """The cells of the half plane that are independent draws with a full complex variance: 0 < kx < nx/2, off the
    ky Nyquist row."""
    m = ~nyquist_mask(ny, nx)
    m[:, 0] = False
    return m


def binned(tqu, res, table, first=100.0, width=200.0, n_min=400):
    """Binned spectra of whole-domain maps against the table's: a list of dicts, one per bin [first + i width,
    first + (i + 1) width) that holds at least ``n_min`` independent cells, with N, the mean over the bin's cells of
    |a_T|^2 / C_TT(ell) and of |a_E|^2 / C_EE(ell) (each cell against its own expectation: unit mean, variance 1/N),
    the mean of Re(a_T a_E*) Lx Ly (``te``), and the bin means of C_TE (``c_te``) and of (C_TT C_EE + C_TE^2) / 2
    (``var_te``: the variance of one cell's Re(a_T a_E*) Lx Ly)."""
    tqu = np.asarray(tqu, np.float64)
    ny, nx = tqu.shape[-2:]
    area = (ny * res) * (nx * res)
    aT, aE, _ = modes_of(tqu, res)
    ell, _, _ = rotation(ny, nx, res)
    cT, cTE, cE, _ = coefficients(table, ell) * np.sqrt(area)
    c_tt, c_te, c_ee = cT * cT, cT * cTE, cTE * cTE + cE * cE
    keep = independent_cells(ny, nx) & (c_tt > 0) & (c_ee > 0)
    out = []
    lo = first
    while lo < ell.max():
        sel = keep & (ell >= lo) & (ell < lo + width)
        n = int(sel.sum())
        if n >= n_min:
            out.append(dict(lo=lo, N=n,
                            tt=float(np.mean(np.abs(aT[sel]) ** 2 * area / c_tt[sel])),
                            ee=float(np.mean(np.abs(aE[sel]) ** 2 * area / c_ee[sel])),
                            te=float(np.mean((aT[sel] * np.conj(aE[sel])).real) * area),
                            c_te=float(np.mean(c_te[sel])),
                            var_te=float(np.mean((c_tt[sel] * c_ee[sel] + c_te[sel] ** 2) / 2))))
        lo += width
    return out


def b_to_e(tqu, res):
    """sum |a_B|^2 / sum |a_E|^2 over EVERY cell of the full plane (fft2, both signs of kx, the Nyquist lines with
    fftfreq's sign).  A cell (kx, -ny/2) of the half plane is read back unchanged by rfft2, whose rotation then finds
    no B in it; its mirror (-kx, -ny/2), which the real field fixes as the conjugate, has sin 2 phi of the other sign
    and holds B = conj(E) sin 4 phi.  Only the full plane shows power left on a Nyquist line."""
    tqu = np.asarray(tqu, np.float64)
    ny, nx = tqu.shape[-2:]
    a = np.fft.fft2(tqu, axes=(-2, -1)) / (ny * nx)
    ky = 2 * np.pi * np.fft.fftfreq(ny, res)[:, None]
    kx = 2 * np.pi * np.fft.fftfreq(nx, res)[None, :]
    k2 = kx * kx + ky * ky
    safe = np.where(k2 > 0, k2, 1.0)
    c2, s2 = np.where(k2 > 0, (kx * kx - ky * ky) / safe, 1.0), np.where(k2 > 0, 2 * kx * ky / safe, 0.0)
    aE, aB = a[1] * c2 + a[2] * s2, -a[1] * s2 + a[2] * c2
    return float((np.abs(aB) ** 2).sum() / (np.abs(aE) ** 2).sum())
