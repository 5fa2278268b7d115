"""The CMB field: flat-sky T, Q, U patches drawn from C_ell on the device (``mrx_cmb_generate``), as a
K_CMB ``ProjectionMap`` that ``Simulation(cmb=...)`` samples into the TOD through the Planck derivative in each band
(the reference: cmb/generation.py:60-103, sim/cmb.py:48).

A spectrum here is ``cl`` [n_ell, 4]: C_ell in K^2, columns TT, EE, BB, TE, row = integer ell from 0.  The measured
spectra are downloads, which this project does not ship: ``read_spectrum`` reads a D_ell text file the user has,
``toy_spectrum`` is a closed-form stand-in."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .map import ProjectionMap

T_CMB = 2.72548  # K (Fixsen 2009)
_H, _KB = 6.62607015e-34, 1.380649e-23
COLUMNS = ("TT", "EE", "BB", "TE")


def kcmb_weight(nu):
    """K_CMB -> K_RJ at ``nu`` (Hz): x^2 e^x / (e^x - 1)^2, x = h nu / (k_B T_CMB), float64."""
    x = _H * np.asarray(nu, np.float64) / (_KB * T_CMB)
    return x * x * np.exp(x) / np.expm1(x) ** 2


def from_dl(ell, dl_uK2):
    """``cl`` [max(ell) + 1, 4] in K^2 from D_ell = ell (ell + 1) C_ell / 2 pi in uK^2, the form CAMB and CLASS write:
    ``ell`` [n] integers, ``dl_uK2`` [n, 4] (TT, EE, BB, TE).  Rows that ``ell`` does not name, and ell = 0, are zero."""
    ell = np.asarray(ell)
    dl = np.asarray(dl_uK2, np.float64)
    if ell.ndim != 1 or dl.shape != (len(ell), 4):
        raise ValueError("ell must be [n] and dl_uK2 [n, 4] (TT, EE, BB, TE)")
    if np.any(ell != np.round(ell)) or np.any(ell < 0):
        raise ValueError("ell must hold non-negative integers")
    ell = ell.astype(np.int64)
    cl = np.zeros((int(ell.max()) + 1, 4))
    keep = ell > 0
    lk = ell[keep].astype(np.float64)
    cl[ell[keep]] = dl[keep] * (2.0 * np.pi / (lk * (lk + 1.0)))[:, None] * 1e-12
    return cl


def to_dl(cl):
    """The inverse of ``from_dl``: ``(ell, dl_uK2)`` of every row of ``cl``."""
    cl = np.asarray(cl, np.float64)
    ell = np.arange(len(cl))
    return ell, cl * (ell * (ell + 1.0) / (2.0 * np.pi))[:, None] * 1e12


def read_spectrum(path):
    """A text file of D_ell in uK^2 with the columns ell, TT, EE, BB, TE (CAMB's ``*_totCls.dat`` / ``*_lensedCls.dat``;
    ``#`` starts a comment; further columns are ignored) -> ``cl``."""
    rows = np.loadtxt(path, comments="#", ndmin=2)
    if rows.shape[1] < 5:
        raise ValueError(f"{path}: expected the columns ell, TT, EE, BB, TE")
    return from_dl(rows[:, 0], rows[:, 1:5])


def toy_spectrum(ell_max=6000, r=0.0):
    """A closed-form STAND-IN with the look of the CMB spectra, not LambdaCDM: damped acoustic peaks 300 apart in
    D_TT (of order 10^3 uK^2), D_EE a few percent of it with its peaks between TT's, C_TE = rho sqrt(C_TT C_EE) with
    rho = 0.6 sin(...) changing sign from peak to trough (|rho| <= 0.9), and BB = 0 unless ``r``: then a bump of
    0.07 r uK^2 around ell = 80.  For tests, examples and timing; science takes ``read_spectrum``."""
    ell = np.arange(int(ell_max) + 1, dtype=np.float64)
    phase = 2.0 * np.pi * (ell - 220.0) / 300.0
    damp = np.exp(-((ell / 1400.0) ** 1.2))
    tt = 1000.0 * damp * (1.6 + np.cos(phase))
    ee = 0.03 * 1000.0 * np.exp(-((ell / 2000.0) ** 1.2)) * (ell / (ell + 300.0)) ** 2 * (1.6 - np.cos(phase))
    te = 0.6 * np.sin(phase) * np.sqrt(tt * ee)
    x = (ell / 80.0) ** 2
    bb = float(r) * 0.07 * x * np.exp(1.0 - x)
    return from_dl(ell, np.stack([tt, ee, bb, te], axis=1))


def spectrum_table(cl, Lx, Ly):
    """The coefficient table ``mrx_cmb_generate`` reads, float32 [n_ell, 4] made in float64: cT = sqrt C_TT,
    cTE = C_TE / sqrt C_TT, cE = sqrt max(C_EE - C_TE^2 / C_TT, 0), cB = sqrt C_BB, each times 1 / sqrt(Lx Ly)
    (``Lx``, ``Ly``: the sides of the periodic domain in radians); the rows ell < 2 are zero.  Raises on a negative
    spectrum or C_TE^2 > C_TT C_EE: no Gaussian field has such spectra."""
    cl = np.asarray(cl, np.float64)
    if cl.ndim != 2 or cl.shape[1] != 4 or len(cl) < 2:
        raise ValueError("cl must be [n_ell, 4] (TT, EE, BB, TE; row = ell) with at least two rows")
    if not np.isfinite(cl).all():
        raise ValueError("cl holds values that are not finite")
    tt, ee, bb, te = cl[2:].T
    if (tt < 0).any() or (ee < 0).any() or (bb < 0).any():
        raise ValueError("negative C_TT, C_EE or C_BB")
    if (te * te > tt * ee * (1.0 + 1e-12)).any():
        bad = int(np.argmax(te * te > tt * ee * (1.0 + 1e-12))) + 2
        raise ValueError(f"C_TE^2 > C_TT C_EE at ell = {bad}: not a covariance")
    table = np.zeros((len(cl), 4))
    root_tt = np.sqrt(tt)
    ok = root_tt > 0
    table[2:, 0] = root_tt
    table[2:, 1] = np.divide(te, root_tt, out=np.zeros_like(te), where=ok)
    table[2:, 2] = np.sqrt(np.maximum(ee - table[2:, 1] ** 2, 0.0))
    table[2:, 3] = np.sqrt(bb)
    return (table / np.sqrt(float(Lx) * float(Ly))).astype(np.float32)


def domain_side(n):
    """The smallest power of two >= 2 n in the transforms' range [64, 8192]."""
    side = 64
    while side < 2 * n:
        side *= 2
    if side > 8192:
        raise ValueError(f"a map side of {n} pixels needs a periodic domain of {side} > 8192: coarsen the resolution or pass domain=")
    return side


def generate_fields(ctx, seed, stream, ny, nx, res, table, out_shape=None, device="cuda:0"):
    """``mrx_cmb_generate``: T, Q, U [3, out_ny, out_nx] float32 on ``device``, the top-left block of the periodic
    ``ny`` x ``nx`` domain of ``res`` radians a pixel, from the float32 [n_ell, 4] ``table`` of ``spectrum_table``."""
    import torch

    from . import _lib
    from ._lib import ptr

    table = np.ascontiguousarray(table, np.float32)
    if table.ndim != 2 or table.shape[1] != 4:
        raise ValueError("table must be [n_ell, 4]")
    oy, ox = out_shape or (ny, nx)
    dev = torch.device(device)
    need = C.c_size_t()
    if _lib.load().mrx_cmb_work_floats(int(ny), int(nx), len(table), C.byref(need)) != _lib.MRX_OK:
        raise ValueError("mrx_cmb_work_floats: sizes must be positive")
    out = torch.empty((3, oy, ox), dtype=torch.float32, device=dev)
    work = torch.empty(need.value, dtype=torch.float32, device=dev)
    fields = (_lib.MrxScreenDesc * 3)()
    for d, plane in zip(fields, out):
        d.d_out, d.out_ny, d.out_nx, d.ld_out = plane.data_ptr(), int(oy), int(ox), 0
    ctx.call("mrx_cmb_generate", int(seed), int(stream), int(ny), int(nx), float(res), table.ctypes.data_as(C.c_void_p),
             len(table), fields, ptr(work), work.numel())
    return out


class CMB(ProjectionMap):
    """One realisation of the CMB on a tangent-plane patch: a ``ProjectionMap`` in K_CMB with one channel (the CMB is
    a temperature: the same at every frequency) that remembers the ``seed`` and the ``spectrum`` it was drawn from."""

    def __init__(self, data, stokes="IQU", seed=None, spectrum=None, **kwargs):
        kwargs.setdefault("nu", 150e9)
        super().__init__(data, stokes=stokes, units="K_CMB", **kwargs)
        self.seed, self.spectrum = seed, spectrum

    @classmethod
    def generate(cls, center=(0.0, 0.0), width=1.0, resolution=1.0 / 60, spectrum=None, seed=None, stokes="IQU",
                 frame="ra/dec", domain=None, device="cuda:0", ctx=None, stream=0):
        """Draw a patch of ``width`` (degrees; a number or (xi, eta) widths) around ``center`` (degrees) at
        ``resolution`` degrees a pixel from ``spectrum`` (``cl``; default ``toy_spectrum()``) with ``seed`` (drawn from
        the system's entropy where None) on the device.  The periodic domain is the smallest power of two >= twice
        the map's side (``domain``: a side or (ny, nx) instead) and the map its top-left block, so that opposite
        edges of the map are not correlated."""
        import torch

        from ._lib import Context

        if not set(stokes) <= set("IQU") or len(set(stokes)) != len(stokes) or not stokes:
            raise ValueError("stokes must be made of 'I', 'Q', 'U'")
        w_xi, w_eta = (width, width) if np.isscalar(width) else width
        if resolution <= 0 or w_xi <= 0 or w_eta <= 0:
            raise ValueError("width and resolution must be positive")
        n_xi, n_eta = (int(np.ceil(w / resolution - 1e-9)) + 1 for w in (w_xi, w_eta))
        if domain is None:
            ny, nx = domain_side(n_eta), domain_side(n_xi)
        else:
            ny, nx = (domain, domain) if np.isscalar(domain) else domain
            if ny < n_eta or nx < n_xi:
                raise ValueError(f"domain {ny} x {nx} smaller than the map {n_eta} x {n_xi}")
        spectrum = toy_spectrum() if spectrum is None else np.asarray(spectrum, np.float64)
        seed = int(seed if seed is not None else np.random.SeedSequence().entropy % (1 << 62))
        res = np.radians(resolution)
        table = spectrum_table(spectrum, nx * res, ny * res)
        dev = torch.device(device)
        torch.cuda.set_device(dev)
        ctx = ctx or Context(dev.index or 0)
        ctx.set_stream(torch.cuda.current_stream(dev))
        tqu = generate_fields(ctx, seed, stream, ny, nx, res, table, (n_eta, n_xi), device=dev).cpu().numpy()
        data = tqu[["IQU".index(s) for s in stokes]][:, None]
        return cls(data, stokes=stokes, seed=seed, spectrum=spectrum, resolution=resolution, center=center, frame=frame)
