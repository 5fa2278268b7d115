"""float64 restatement of the detector noise mrx_noise_generate defines, draw for draw.
TEST INFRASTRUCTURE ONLY (see oracle/hotpath.py).

Built from the documented model (maria_amd/csrc/mrx_noise.hip's header, include/mrx.h), not from
the kernels' loops.  The discrete choices are inputs taken from the library: the Philox counters
and tags below, the cell layout k = k1 + n1 k2, the period (n1, n2) of mrx_noise_period,
k_min = ceil(N / T), k_cut = min(64 k_min, N / 2) and the series id 16 + global_row / 2 of a pair
of rows.  Everything else is float64 numpy: Philox-4x32-10 on uint64 arrays, Box-Muller with the
exact logarithm, sine and cosine, numpy's inverse FFT, the window mean in closed form.

One-rate form, per pair of rows (a, b = a + 1), N = n1 n2, |k| = min(k, N - k):
  * own cells: X[k] = sqrt(fs/N + (1-c) knee/|k|) g[k] for |k| >= k_cut, and
    X[k] = sqrt((1-c) knee/|k|) g[k] + sqrt(fs/N) h[k] below it; the pink term is 0 below k_min.
    g: counter (k1, k2 mod n2/2, series, 'PINK'), words (x, y) for k2 < n2/2, (z, w) above;
    h: the same counters with the tag 'WHT2'.
  * modes: X[k] += sqrt(c) (B[a,m] + i B[b,m]) F_m[k], F_m Hermitian, cell |k| drawn at
    (|k|, m, 0, 'MODE'): white sqrt(fs/N) from words (x, y), pink sqrt(knee/|k|) from (z, w)
    (each halved in variance per component off the self-conjugate cells 0 and N/2, which are real).
  * x = N ifft(X); the window mean over t < T of the pink parts of the cells k_min <= |k| < k_cut is
    subtracted; Re x is row a, Im x row b (a lone last row keeps Re only).
  c is corr_prop when the call has modes and 0 without (the generator has nothing to correlate).
White only (knee = 0): sqrt(fs) BM(philox(t >> 2, det_offset + row, t >> 34, 'WHIT')), sample t % 4 of
the four normals.  Two-rate form: see two_rate.  Every form then takes the level
scale + per_loading * loading and is added to the output when accumulating (level()).
"""

from __future__ import annotations

import numpy as np

TAG_PINK = 0x50494E4B  # 'PINK': a pair's own cells
TAG_WHT2 = 0x57485432  # 'WHT2': the white part of a pair's cells below k_cut
TAG_MODE = 0x4D4F4445  # 'MODE': the modes' Hermitian spectra
TAG_WHIT = 0x57484954  # 'WHIT': a row's per-sample white draws (white-only and two-rate forms)
TAG_MWHM = 0x4D57484D  # 'MWHM': the modes' per-sample white series (two-rate form)
SERIES0 = 16  # detector pair (2q, 2q + 1) is series 16 + q

# tests/test_gpu_noise_philox.py: max_t |kernel - rebuild| / rms(row), every row of every case, stays below this.
# Four times the largest ratio measured on an MI355X over all its cases (1.9e-5: see that file); every mistake of
# tests/test_host_noise_philox.py moves the output by 30 times this or more.
GPU_BOUND = 7.5e-5

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, seed):
    """Philox-4x32-10 (Salmon et al. 2011) on arrays of counter words; key = (seed low, seed high).
    Returns the four output words as uint64 arrays (values < 2^32)."""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = 0x9E3779B9, 0xBB67AE85
    s32 = np.uint64(32)
    x, y, z, w = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * x
        p1 = M1 * z
        x, y, z, w = (p1 >> s32) ^ y ^ np.uint64(k0), p1 & _M32, (p0 >> s32) ^ w ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return x, y, z, w


def box_muller(a, b, swap=False):
    """Two unit normals from two Philox words as one complex number (mrx_spectral.h: box_muller):
    u1 = ((a >> 8) + 0.5) / 2^24 in (0, 1), u2 = (b >> 8) / 2^24, sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2).
    ``swap``: sine and cosine exchanged (a perturbation for the tests)."""
    u1 = ((a >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = (b >> np.uint64(8)).astype(np.float64) / 16777216.0
    rad = np.sqrt(-2.0 * np.log(u1))
    c, s = np.cos(2 * np.pi * u2), np.sin(2 * np.pi * u2)
    if swap:
        c, s = s, c
    return rad * c + 1j * rad * s


def window(n, T):
    """(k_min, k_cut): nothing slower than the TOD, and the cells that carry the pink window mean."""
    k_min = -(-n // T)
    return k_min, min(64 * k_min, n // 2)


def window_mean_factor(k, n, T):
    """W_k / T, W_k = sum_{t<T} exp(2 pi i k t / N), for integer k != 0 mod N (closed form; phases reduced mod 2N exactly)."""
    k = np.asarray(k, dtype=np.int64)
    a = ((k * (T - 1)) % (2 * n)) / n
    b = ((k * T) % (2 * n)) / n
    s = np.sin(np.pi * (k % (2 * n)) / n)
    return np.exp(1j * np.pi * a) * np.sin(np.pi * b) / (T * s)


def _draw_grid(n1, n2, c2, tag, seed, swap=False):
    """Complex normals of every cell k = k1 + n1 k2 of a pair's spectrum (length n1 n2): counter
    (k1, k2 mod n2/2, c2, tag), words (x, y) for k2 < n2/2 and (z, w) for the upper half."""
    half = n2 // 2
    k1 = np.arange(n1, dtype=np.uint64)[None, :]
    k2 = np.arange(half, dtype=np.uint64)[:, None]
    x, y, z, w = philox4x32(k1, k2, c2, tag, seed)
    g = np.empty((n2, n1), complex)  # [k2][k1]: k = k1 + n1 k2 in row-major order
    g[:half] = box_muller(x, y, swap)
    g[half:] = box_muller(z, w, swap)
    return g.reshape(-1)


def _draw_cells(k, n1, n2, c2, tag, seed, swap=False):
    """The same normals for the listed cells only."""
    k = np.asarray(k, dtype=np.int64)
    half = n2 // 2
    k1, k2 = k % n1, k // n1
    up = k2 >= half
    x, y, z, w = philox4x32(k1.astype(np.uint64), (k2 - half * up).astype(np.uint64), c2, tag, seed)
    return np.where(up, box_muller(z, w, swap), box_muller(x, y, swap))


def mode_spectra(seed, n_modes, n1, n2, white_var, knee, k_min, perturb=(), swap=False):
    """F[m][k] (Hermitian) and its pink part alone: cell |k| drawn at (|k|, m, 0, 'MODE')."""
    n = n1 * n2
    kk = np.arange(n // 2 + 1)
    F = np.zeros((n_modes, n), complex)
    Fp = np.zeros((n_modes, n), complex)
    self_conj = (kk == 0) | (2 * kk == n)
    var_p = np.where(kk >= k_min, knee / np.maximum(kk, 1), 0.0)
    for m in range(n_modes):
        x, y, z, w = philox4x32(kk.astype(np.uint64), m, 0, TAG_MODE, seed)
        hw, hp = box_muller(x, y, swap), box_muller(z, w, swap)
        half_w = np.where(self_conj, hw.real, hw / np.sqrt(2))
        half_p = np.where(self_conj, hp.real, hp / np.sqrt(2))
        pink = np.sqrt(var_p) * half_p
        both = np.sqrt(white_var) * half_w + pink
        for dst, v in ((F[m], both), (Fp[m], pink)):
            dst[: n // 2 + 1] = v
            mirror = v[1 : n // 2][::-1]  # the cells N - |k|: the conjugates (perturbed: the imaginary sign kept)
            dst[n // 2 + 1 :] = mirror if "mode_upper_sign" in perturb else np.conj(mirror)
    return F, Fp


def one_rate(seed, D, T, fs, knee, n1, n2, corr=0.0, basis=None, det_offset=0, white=True, perturb=(), keep=None):
    """Unscaled noise [D, T] of the one-rate form (float64).  ``white=False``: no white part in the
    spectrum (the two-rate form's slow series).  ``keep``: samples returned (default T; N: the whole
    period, the window mean still the one over the first T).  ``perturb``: names of deliberate mistakes, for the
    sensitivity tests (mode_upper_sign, no_window_mean, k_min_minus_1, swap_cos_sin, cell)."""
    n = n1 * n2
    n_modes = 0 if basis is None else basis.shape[1]
    c = corr if n_modes > 0 else 0.0
    k_min, k_cut = window(n, T)
    if "k_min_minus_1" in perturb:
        k_min -= 1
    swap = "swap_cos_sin" in perturb
    white_var = fs / n if white else 0.0
    k = np.arange(n)
    kk = np.minimum(k, n - k)
    pink_var = np.where(kk >= k_min, (1.0 - c) * knee / np.maximum(kk, 1), 0.0)
    low = np.nonzero(kk < k_cut)[0]
    win = np.nonzero((kk >= k_min) & (kk < k_cut))[0]
    Wt = window_mean_factor(win, n, T)
    if n_modes:
        F, Fp = mode_spectra(seed, n_modes, n1, n2, white_var, knee, k_min, perturb, swap)
        B = np.asarray(basis, np.float64)
    amp_hi = np.sqrt(white_var + pink_var)
    keep = T if keep is None else keep
    out = np.empty((D, keep))
    for a in range(0, D, 2):
        has_b = a + 1 < D
        series = SERIES0 + (det_offset + a) // 2
        g = _draw_grid(n1, n2, series, TAG_PINK, seed, swap)
        X = amp_hi * g
        h = _draw_cells(low, n1, n2, series, TAG_WHT2, seed, swap)
        X[low] = np.sqrt(pink_var[low]) * g[low] + np.sqrt(white_var) * h
        P = np.sqrt(pink_var[win]) * g[win]  # the pink parts of the window-mean cells
        if n_modes:
            coef = np.sqrt(c) * (B[a] + (1j * B[a + 1] if has_b else 0.0))
            X += coef @ F
            P = P + coef @ Fp[:, win]
        if "cell" in perturb:  # one cell above k_cut, where the white part dominates: the smallest change
            X[n // 2 - 5] *= -1.0
        x = np.fft.ifft(X)[:keep] * n
        if "no_window_mean" not in perturb:
            x = x - np.sum(P * Wt)
        out[a] = x.real
        if has_b:
            out[a + 1] = x.imag
    return out


def _sample_normals(T, ids, tag, seed):
    """[len(ids), T] unit normals of the per-sample series: sample t of series id is normal t % 4 of
    philox(t >> 2, id, t >> 34, tag) = (Re, Im of BM(x, y), Re, Im of BM(z, w))."""
    q = np.arange((T + 3) // 4, dtype=np.uint64)[None, :]
    ids = np.asarray(list(ids), dtype=np.uint64)[:, None]
    x, y, z, w = philox4x32(q, ids, q >> np.uint64(32), tag, seed)
    g0, g1 = box_muller(x, y), box_muller(z, w)
    return np.stack([g0.real, g0.imag, g1.real, g1.imag], axis=2).reshape(len(ids), -1)[:, :T]


def white_only(seed, D, T, fs, det_offset=0):
    """Unscaled white noise of the knee = 0 path, [D, T]."""
    return np.sqrt(fs) * _sample_normals(T, range(det_offset, det_offset + D), TAG_WHIT, seed)


def catmull_rom_weights(u):
    """Weights of (P[-1], P[0], P[1], P[2]) at u in [0, 1)."""
    u = np.asarray(u, np.float64)
    return np.stack([0.5 * (-u**3 + 2 * u**2 - u), 0.5 * (3 * u**3 - 5 * u**2 + 2), 0.5 * (-3 * u**3 + 4 * u**2 + u),
                     0.5 * (u**3 - u**2)])


def two_rate(seed, D, T, fs, knee, rate, n1s, n2s, corr=0.0, basis=None, det_offset=0, perturb=()):
    """Unscaled noise [D, T] of the two-rate form:
      1. the one-rate form's slow series: T_s = ceil(T / rate) + 4 samples at fs / rate, no white part;
      2. the four-point Catmull-Rom cubic at u = r / rate: sample t = rate s + r reads slow samples s .. s + 3;
      3. + sqrt(fs) w[row, t], the white-only path's draws;
      4. + sqrt(c) sqrt(fs) sum_m B[row, m] MW[m][t], MW drawn at (t >> 2, m, 0, 'MWHM').
    (n1s, n2s): mrx_noise_period(T_s).  ``perturb`` 'cr_phase': the cubic at u = (r + 1) / rate."""
    Ts = -(-T // rate) + 4
    lo = one_rate(seed, D, Ts, fs / rate, knee, n1s, n2s, corr, basis, det_offset, white=False, perturb=perturb)
    t = np.arange(T)
    s, r = t // rate, t % rate
    u = (r + (1 if "cr_phase" in perturb else 0)) / rate
    w = catmull_rom_weights(u)
    x = sum(w[j] * lo[:, s + j] for j in range(4))
    x += white_only(seed, D, T, fs, det_offset)
    if basis is not None and basis.shape[1] > 0:
        mw = _sample_normals(T, range(basis.shape[1]), TAG_MWHM, seed)
        x += np.sqrt(corr) * np.sqrt(fs) * (np.asarray(basis, np.float64) @ mw)
    return x


def two_rate_factor(T, fs, knee, one_rate_only=False):
    """The rate the library picks (mrx_noise.hip: two_rate_factor): 4 or 2 where the pink part at the slow
    Nyquist frequency stays below 2 % of the white level and T >= 32768, else 1."""
    if one_rate_only or not knee > 0 or T < 32768:
        return 1
    for rate in (4, 2):
        if 2.0 * rate * knee / fs <= 0.0205:
            return rate
    return 1


def level(x, scale=None, loading=None, per_loading=0.0, base=None):
    """The epilogue: x (scale + per_loading loading) [+ base when accumulating]."""
    amp = np.ones((x.shape[0], 1)) if scale is None else np.asarray(scale, np.float64)[:, None]
    if loading is not None:
        amp = amp + per_loading * np.asarray(loading, np.float64)
    y = x * amp
    return y if base is None else y + np.asarray(base, np.float64)


def generate(seed, D, T, fs, knee, period, corr=0.0, basis=None, det_offset=0, one_rate_only=False, perturb=()):
    """What mrx_noise_generate writes before the level is applied, [D, T] float64.
    ``period(T) -> (n1, n2)``: the library's mrx_noise_period."""
    if not knee > 0:
        return white_only(seed, D, T, fs, det_offset)
    rate = two_rate_factor(T, fs, knee, one_rate_only)
    if rate > 1:
        n1, n2 = period(-(-T // rate) + 4)
        return two_rate(seed, D, T, fs, knee, rate, n1, n2, corr, basis, det_offset, perturb)
    n1, n2 = period(T)
    return one_rate(seed, D, T, fs, knee, n1, n2, corr, basis, det_offset, perturb=perturb)


def row_ratios(got, ref, base=None):
    """Per row: max_t |got - ref| / rms of the row's noise (ref, less ``base`` when the noise was added to one)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    noise = ref if base is None else ref - np.asarray(base, np.float64)
    return np.max(np.abs(got - ref), axis=1) / np.sqrt(np.mean(noise**2, axis=1))
