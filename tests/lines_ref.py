"""The numpy float64 reference of maria_amd.lines: the basis and the two formulas of include/mrx.h with their
operation order, ``solve`` (regress_ref's), the line finder, the phase-slope refinement and TOD.remove_lines' steps, plain
and slow.  Sums are ``math.fsum`` over the rounded products: the correctly rounded sum, whatever order the device adds in.

cospi and sinpi are written by exact octant reduction: x = n / 2 + r with n = rint(2 x) and |r| <= 1 / 4 exactly, the two
functions of pi r evaluated in long double (64 mantissa bits where the platform has them) and rounded once to float64,
then signs and places swapped by n mod 4.  At the quarter cycles r = 0, so the values are exactly 0 and +-1 (numpy's
cos(pi / 2) is 6e-17).  Where long double is float64 the values carry libm's rounding and the rounding of pi r: within one
ulp, the allowance the device tests give the reference."""

import functools
import math

import numpy as np
import regress_ref
import subscans_ref

LONG = np.longdouble
PI_LONG = LONG(3.141592653589793) + LONG(1.2246467991473532e-16)  # pi = hi + lo, exact to the long double's rounding
HAS_LONG = np.finfo(LONG).eps < 2.0**-60

segments = subscans_ref.segments


def sincospi(x):
    """(sinpi(x), cospi(x)) of a float64 array, each within one rounding of the exact value (with long double)."""
    x = np.asarray(x, np.float64)
    finite = np.isfinite(x)
    x = np.where(finite, x, 0.0)
    n = np.rint(2.0 * x)
    r = x - 0.5 * n  # exact: |r| <= 1 / 4 on x's own grid
    arg = PI_LONG * r.astype(LONG)
    s, c = np.sin(arg).astype(np.float64), np.cos(arg).astype(np.float64)
    s = np.where(r == 0.0, 0.0, s)
    c = np.where(r == 0.0, 1.0, c)
    k = np.mod(n, 4.0).astype(np.int64)
    sin = np.choose(k, [s, c, -s, -c])
    cos = np.choose(k, [c, -s, -c, s])
    return np.where(finite, sin, np.nan) + 0.0, np.where(finite, cos, np.nan) + 0.0


def reduced_phase(nu, t):
    """q = theta - rint(theta), theta = nu * float64(t): [.., n] for nu [..] and the sample indices t [n]."""
    theta = np.asarray(nu, np.float64)[..., None] * np.asarray(t, np.int64).astype(np.float64)
    return theta - np.rint(theta)


def carriers(nu, t):
    """(cos, sin) [.., n] of the lines ``nu`` [..] at the samples ``t`` [n] counted from the start of the row."""
    q = reduced_phase(nu, t)
    s, c = sincospi(2.0 * q)
    return c, s


def basis(lo, hi, nu_row, n_poly):
    """[K, hi - lo] float64: B_0 .. B_{K - 1} of one row on the segment [lo, hi), operation for operation."""
    n = hi - lo
    L = len(nu_row)
    B = np.empty((n_poly + 2 * L, n))
    if n_poly:
        B[:n_poly] = subscans_ref.basis(n, 2)[:n_poly]
    c, s = carriers(np.asarray(nu_row, np.float64), np.arange(lo, hi))
    B[n_poly::2], B[n_poly + 1::2] = c, s
    return B


def _terms(x, model):
    t = np.asarray(x, np.float32).astype(np.float64)
    return t if model is None else t - np.asarray(model, np.float32).astype(np.float64)


def _nu(nu, D):
    nu = np.asarray(nu, np.float64)
    return np.broadcast_to(nu[None, :], (D, nu.size)) if nu.ndim == 1 else nu


def normal_equations(x, bounds, nu, n_poly, flags=None, model=None):
    """(N [D, S, K, K], r [D, S, K], hits [D, S] int64, absN, absr, dN, dr): fsum of the rounded products over the kept
    samples; the sums of the products' magnitudes (for the rounding bound); and the sums of |d term / d carrier| (for the
    carriers' own error): |term(d, t)| for r_i with B_i a carrier, |B_j| (+ |B_i|) for N_ij with B_i (and B_j) a carrier."""
    terms = _terms(x, model)
    D, T = terms.shape
    nu = _nu(nu, D)
    K = n_poly + 2 * nu.shape[1]
    segs = segments(bounds, T)
    S = len(segs)
    N, r, hits = np.zeros((D, S, K, K)), np.zeros((D, S, K)), np.zeros((D, S), np.int64)
    aN, ar, dN, dr = np.zeros((D, S, K, K)), np.zeros((D, S, K)), np.zeros((D, S, K, K)), np.zeros((D, S, K))
    wave = np.arange(K) >= n_poly
    for s, (lo, hi) in enumerate(segs):
        if hi <= lo:
            continue
        for d in range(D):
            keep = np.ones(hi - lo, bool) if flags is None else np.asarray(flags)[d, lo:hi] == 0
            b, y = basis(lo, hi, nu[d], n_poly)[:, keep], terms[d, lo:hi][keep]
            mag = [math.fsum(np.abs(b[i])) for i in range(K)]
            for i in range(K):
                for j in range(i, K):
                    p = b[i] * b[j]
                    N[d, s, i, j] = N[d, s, j, i] = math.fsum(p)
                    aN[d, s, i, j] = aN[d, s, j, i] = math.fsum(np.abs(p))
                    dN[d, s, i, j] = dN[d, s, j, i] = wave[i] * mag[j] + wave[j] * mag[i]
                p = b[i] * y
                r[d, s, i], ar[d, s, i] = math.fsum(p), math.fsum(np.abs(p))
                dr[d, s, i] = wave[i] * math.fsum(np.abs(y))
            hits[d, s] = int(keep.sum())
    return N, r, hits, aN, ar, dN, dr


def fit_values(bounds, nu, a, n_poly, T):
    """[D, T] float64: s = ((0 + a_c cos) + a_s sin) + .. over the carriers of every sample's segment; 0 in no segment."""
    a = np.asarray(a, np.float64)
    D, S, K = a.shape
    nu = _nu(nu, D)
    out = np.zeros((D, T))
    for s, (lo, hi) in enumerate(segments(bounds, T)):
        if hi <= lo:
            continue
        c, sn = carriers(nu, np.arange(lo, hi))  # [D, L, n]
        acc = np.zeros((D, hi - lo))
        for l in range(nu.shape[1]):
            acc = acc + a[:, s, n_poly + 2 * l, None] * c[:, l]
            acc = acc + a[:, s, n_poly + 2 * l + 1, None] * sn[:, l]
        out[:, lo:hi] = acc
    return out


def covered(bounds, T):
    m = np.zeros(T, bool)
    for lo, hi in segments(bounds, T):
        m[lo:hi] = True
    return m


def apply(x, bounds, nu, a, n_poly, sign=-1):
    """y = x + sign * float32(s) inside the segments, x elsewhere."""
    x = np.asarray(x, np.float32)
    D, T = x.shape
    f = fit_values(bounds, nu, a, n_poly, T).astype(np.float32)
    y = np.where(covered(bounds, T)[None, :], x - f if sign < 0 else x + f, x)
    return y.astype(np.float32)


def fit(x, bounds, nu, n_poly, flags=None, model=None, min_hits=8, rcond=1e-10):
    """(a [D, S, K], ok [D, S]): regress_ref.solve of every (row, segment)."""
    N, r, hits = normal_equations(x, bounds, nu, n_poly, flags=flags, model=model)[:3]
    D, S = hits.shape
    K = r.shape[2]
    a, ok = regress_ref.solve(N.reshape(D * S, K, K), r.reshape(D * S, K), hits.reshape(D * S), min_hits=min_hits, rcond=rcond)
    return a.reshape(D, S, K), ok.reshape(D, S)


def fit_fast(x, bounds, nu, n_poly, flags=None, model=None, min_hits=8, rcond=1e-10):
    """``fit`` with numpy's pairwise sums in place of fsum (N and r within n 2^-53 sum|terms| of it): for the pipeline at
    the science fixture's size, where the fsum loops take minutes."""
    terms = _terms(x, model)
    D, T = terms.shape
    nu = _nu(nu, D)
    K = n_poly + 2 * nu.shape[1]
    segs = segments(bounds, T)
    S = len(segs)
    N, r, hits = np.zeros((D, S, K, K)), np.zeros((D, S, K)), np.zeros((D, S), np.int64)
    for s, (lo, hi) in enumerate(segs):
        for d in range(D if hi > lo else 0):
            keep = np.ones(hi - lo, bool) if flags is None else np.asarray(flags)[d, lo:hi] == 0
            b, y = basis(lo, hi, nu[d], n_poly)[:, keep], terms[d, lo:hi][keep]
            N[d, s], r[d, s], hits[d, s] = (b[:, None, :] * b[None, :, :]).sum(axis=2), (b * y[None, :]).sum(axis=1), keep.sum()
    a, ok = regress_ref.solve(N.reshape(D * S, K, K), r.reshape(D * S, K), hits.reshape(D * S), min_hits=min_hits, rcond=rcond)
    return a.reshape(D, S, K), ok.reshape(D, S)


def amplitude_phase(a, n_poly):
    a = np.asarray(a, np.float64)
    c, s = a[:, :, n_poly::2], a[:, :, n_poly + 1::2]
    return np.hypot(c, s), np.arctan2(-s, c)


# ---- the finder ----

def running_median(y, h):
    y = np.asarray(y, np.float64)
    out = np.empty(y.size)
    for i in range(y.size):
        idx = np.clip(np.arange(i - h, i + h + 1), 0, y.size - 1)  # the ends repeated
        out[i] = np.median(y[idx])
    return out


def find_lines(f, psd, groups=None, n_sigma=6.0, half_window=16, f_min=None, f_max=None, max_lines=None):
    """A list of frequency arrays, one a group, strongest first: maria_amd.lines.find_lines step for step, with loops."""
    f, p = np.asarray(f, np.float64), np.atleast_2d(np.asarray(psd, np.float64))
    F, h = f.size, int(half_window)
    g = np.zeros(p.shape[0], np.int64) if groups is None else np.asarray(groups, np.int64)
    out = []
    for k in range(int(g.max()) + 1):
        rows = p[g == k]
        if rows.shape[0] == 0:
            out.append(np.zeros(0))
            continue
        spec = np.median(rows / np.median(rows, axis=1, keepdims=True), axis=0)
        y = np.log(np.maximum(spec, np.finfo(np.float64).tiny))
        base = running_median(y, h)
        z = y - base
        zi = z[h:F - h]
        sigma = 1.4826 * np.median(np.abs(zi - np.median(zi)))
        lines, i = [], h
        while i < F - h:
            ok = z[i] > n_sigma * sigma and (f_min is None or f[i] >= f_min) and (f_max is None or f[i] <= f_max)
            if not ok:
                i += 1
                continue
            j = i
            while j + 1 < F - h and z[j + 1] > n_sigma * sigma and (f_max is None or f[j + 1] <= f_max):
                j += 1
            a, b = max(i - 1, 0), min(j + 1, F - 1)
            w = np.maximum(np.exp(y[a:b + 1]) - np.exp(base[a:b + 1]), 0.0)
            lines.append((float(z[i:j + 1].max()), float((w * f[a:b + 1]).sum() / w.sum())))
            i = j + 1
        lines.sort(key=lambda v: -v[0])
        out.append(np.array([v for _, v in (lines if max_lines is None else lines[:max_lines])], np.float64))
    return out


# ---- the refinement ----

def phase_slope(a, ok, bounds, T, n_poly, groups=None, per_detector=True):
    """[D, L]: per row the median over consecutive pairs of non-empty, fitted segments of the wrapped phase difference
    divided by 2 pi times the distance of the segments' centres; per group its rows' median with ``per_detector`` False."""
    _, phi = amplitude_phase(a, n_poly)
    D, S, L = phi.shape
    segs = [(s, (lo + hi - 1) / 2.0) for s, (lo, hi) in enumerate(segments(bounds, T)) if hi > lo]
    out, have = np.zeros((D, L)), np.zeros(D, bool)
    for d in range(D):
        steps = []
        for (s0, c0), (s1, c1) in zip(segs[:-1], segs[1:]):
            if ok[d, s0] and ok[d, s1]:
                dphi = phi[d, s1] - phi[d, s0]
                dphi = dphi - 2.0 * np.pi * np.floor(dphi / (2.0 * np.pi) + 0.5)
                steps.append(dphi / (2.0 * np.pi * (c1 - c0)))
        if steps:
            out[d], have[d] = np.median(np.array(steps), axis=0), True
    if not per_detector:
        g = np.zeros(D, np.int64) if groups is None else np.asarray(groups, np.int64)
        for k in np.unique(g[g >= 0]):
            rows = (g == k) & have
            if rows.any():
                out[g == k] = np.median(out[rows], axis=0)
    return out


def refine(x, bounds, nu, n_iter=2, per_detector=True, n_poly=1, flags=None, model=None, groups=None, min_hits=8, rcond=1e-10, fit=fit):
    x = np.asarray(x, np.float32)
    D, T = x.shape
    nu = np.array(_nu(nu, D), np.float64)
    for _ in range(n_iter):
        a, ok = fit(x, bounds, nu, n_poly, flags=flags, model=model, min_hits=min_hits, rcond=rcond)
        nu = np.clip(nu + phase_slope(a, ok, bounds, T, n_poly, groups=groups, per_detector=per_detector), np.finfo(np.float64).tiny, 0.5)
    return nu


# ---- the front end ----

def chunk_bounds(T, length):
    return np.append(np.arange(0, T, length), T).astype(np.int32)


def line_groups(n):
    return [list(range(lo, min(lo + 3, n))) for lo in range(0, n, 3)]


def remove_lines(signal, into, fs, lines=None, chunk=None, n_poly=2, n_sigma=6.0, nperseg=2048, n_refine=2, per_detector=True, groups=None,
                 flags=None, model=None, min_hits=None, rcond=1e-10, fit=fit_fast):
    """(y, record): TOD.remove_lines on the host.  The spectrum is scipy.signal.welch of the float32 signal less the model
    in float64; per group of rows the lines are found (or given, in Hz), sorted, and taken in sets of three neighbours:
    refined and fitted on the working signal from which the earlier sets are already gone, subtracted from it and from
    ``into``, every step rounded to float32 where the front end rounds it."""
    import scipy.signal

    signal = np.asarray(signal, np.float32)
    D, T = signal.shape
    work = signal if model is None else (signal - np.asarray(model, np.float32)).astype(np.float32)
    y = np.array(into, np.float32)
    g = np.zeros(D, np.int64) if groups is None else np.asarray(groups, np.int64)
    length = int(nperseg) if chunk is None else int(round(chunk * fs))
    bounds = chunk_bounds(T, length)
    S = len(bounds) - 1
    if lines is None:
        f, p = scipy.signal.welch(work.astype(np.float64), fs, nperseg=nperseg)
        found = find_lines(f, p, groups=g, n_sigma=n_sigma)
    else:
        found = [np.asarray(lines, np.float64)] * (int(g.max()) + 1)
    Lmax = max([v.size for v in found] + [0])
    rec = {"found": np.full((D, Lmax), np.nan), "refined": np.full((D, Lmax), np.nan), "amplitude": np.full((D, S, Lmax), np.nan),
           "phase": np.full((D, S, Lmax), np.nan), "unfitted": 0, "lines": found}
    nonempty = np.diff(bounds) > 0
    for k, freqs in enumerate(found):
        rows = np.flatnonzero(g == k)
        if rows.size == 0 or freqs.size == 0:
            continue
        order = np.argsort(freqs)
        rec["found"][np.ix_(rows, np.arange(freqs.size))] = freqs[None, :]
        w = work[rows].copy()
        fl = None if flags is None else np.asarray(flags)[rows]
        for members in line_groups(freqs.size):
            cols = order[members]
            nu0 = freqs[cols] / fs
            K = n_poly + 2 * len(cols)
            mh = 4 * K if min_hits is None else min_hits
            nu = refine(w, bounds, nu0, n_iter=n_refine, per_detector=per_detector, n_poly=n_poly, flags=fl, min_hits=mh, rcond=rcond, fit=fit)
            a, ok = fit(w, bounds, nu, n_poly, flags=fl, min_hits=mh, rcond=rcond)
            w = apply(w, bounds, nu, a, n_poly)
            y[rows] = apply(y[rows], bounds, nu, a, n_poly)
            amp, phi = amplitude_phase(a, n_poly)
            rec["refined"][np.ix_(rows, cols)] = nu * fs
            rec["amplitude"][np.ix_(rows, np.arange(S), cols)] = amp
            rec["phase"][np.ix_(rows, np.arange(S), cols)] = phi
            rec["unfitted"] += int((~ok & nonempty[None, :]).sum())
    return y, rec


def noise_floor(n_lines, bounds, T, sigma, injected_rms):
    """The rms that white noise of ``sigma`` leaves in a fit of 2 L free amplitudes per chunk, as a fraction of the
    injected rms: each parameter absorbs sigma^2 / n of a chunk's variance per sample, so the fitted carriers differ from
    the true ones by sigma sqrt(2 L S / T) rms over S chunks of T / S samples on average."""
    S = int((np.diff(np.clip(bounds, 0, T)) > 0).sum())
    return sigma * math.sqrt(2.0 * n_lines * S / T) / injected_rms


# ---- the science fixture ----

FS, LINE_HZ, LINE_AMP, SCATTER = 100.0, (7.3137, 21.947), (0.5, 0.3), 1e-4


@functools.lru_cache(maxsize=None)
def science_case(D=12, T=24000, seed=5, lines=LINE_HZ, amps=LINE_AMP, scatter=SCATTER, drift=0.02):
    """(x, clean, true_hz, injected_rms): white noise of sigma 1 plus a random-walk drift (``drift`` a step) in ``clean``,
    and in ``x`` the lines on top, each detector's frequencies scattered by ``scatter`` (relative, Gaussian) and its phases
    random; both float32 [D, T] at 100 Hz.  ``injected_rms``: the rms of the injected lines."""
    rng = np.random.default_rng(seed)
    clean = rng.standard_normal((D, T)) + np.cumsum(drift * rng.standard_normal((D, T)), axis=1)
    hz = np.asarray(lines)[None, :] * (1.0 + scatter * rng.standard_normal((D, len(lines))))
    phase = rng.uniform(-np.pi, np.pi, (D, len(lines)))
    t = np.arange(T) / FS
    wave = sum(amps[l] * np.cos(2.0 * np.pi * hz[:, l, None] * t[None, :] + phase[:, l, None]) for l in range(len(lines)))
    x, clean = (clean + wave).astype(np.float32), clean.astype(np.float32)
    for v in (x, clean, hz):
        v.setflags(write=False)
    return x, clean, hz, float(np.sqrt((wave**2).mean()))
