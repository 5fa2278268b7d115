"""The float64 reference of mrx_tod_onepole and mrx_tod_onepole_inverse (include/mrx.h) in numpy, the inputs
the tests share, and a blocked scan with the mistakes a time-parallel kernel can make.

    lag       g = 1.0 - a;  y64[0] = init ? x[0] : g x[0];  y64[t] = a y64[t - 1] + g x[t]        (serial, float64)
    inverse   r = 1.0 / (1.0 - a);  x[0] = init ? y[0] : float32(y[0] r);  x[t] = float32((y[t] - a y[t - 1]) r)

numpy multiplies and adds float64 arrays one rounding an operation (no fused multiply-add), which is what the header asks
of the kernels.  A row whose a is not in (0, 1) is copied."""

import functools

import numpy as np

POLES = [0.0, 2.0**-10, 0.5, 0.78, 1.0 - 2.0**-8, 1.0 - 2.0**-12]
ROWS = [1, 3, 33]
TIMES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099, 10007]
TILE = 1024


def lagged(a):
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore"):
        return (a > 0.0) & (a < 1.0)


def forward64(x, a, init):
    """[D, T] float64: the serial recurrence of every row of ``x`` [D, T] float32 with the poles ``a`` [D]."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    a = np.asarray(a, np.float64)
    on = lagged(a)
    aa = np.where(on, a, 0.0)[:, None]
    g = 1.0 - aa
    y = np.empty_like(x64)
    y[:, 0] = x64[:, 0] if init else g[:, 0] * x64[:, 0]
    for t in range(1, x64.shape[1]):
        y[:, t] = aa[:, 0] * y[:, t - 1] + g[:, 0] * x64[:, t]
    y[~on] = x64[~on]
    return y


def inverse(y, a, init):
    """[D, T] float32: the two-tap FIR of every row of ``y`` [D, T] float32, operation by operation."""
    y = np.asarray(y, np.float32)
    y64 = y.astype(np.float64)
    a = np.asarray(a, np.float64)
    on = lagged(a)
    aa = np.where(on, a, 0.0)[:, None]
    r = 1.0 / (1.0 - aa)
    x = np.empty_like(y)
    x[:, 0] = y[:, 0] if init else (y64[:, 0] * r[:, 0]).astype(np.float32)
    x[:, 1:] = ((y64[:, 1:] - aa * y64[:, :-1]) * r).astype(np.float32)
    x[~on] = y[~on]
    return x


def forward_bound(y64, x, a):
    """The per-sample bound of the lag's float32 result against ``y64``: 2^-24 |y64| (the float32 store) +
    64 2^-53 max|x| / (1 - a) (the float64 roundings of any association order)."""
    return 2.0**-24 * np.abs(y64) + float64_term(x, a)


def float64_term(x, a):
    """[D, 1]: 64 2^-53 max|x| / (1 - a), the part of ``forward_bound`` that a float64 result is held to (0 for a copied
    row)."""
    a = np.asarray(a, np.float64)
    on = lagged(a)
    peak = np.abs(np.asarray(x, np.float64)).max(axis=1)
    return np.where(on, 64.0 * 2.0**-53 * peak / (1.0 - np.where(on, a, 0.0)), 0.0)[:, None]


def round_trip_bound(x, y, a):
    """The per-sample bound of inverse(lag(x)) against x: 2^-24 |x| + (1 + a) / (1 - a) 2^-23 max|y|."""
    a = np.where(lagged(a), np.asarray(a, np.float64), 0.0)
    peak = np.abs(np.asarray(y, np.float64)).max(axis=1)
    return 2.0**-24 * np.abs(np.asarray(x, np.float64)) + ((1.0 + a) / (1.0 - a) * 2.0**-23 * peak)[:, None]


def poles_of(D, seed):
    """[D] float64: POLES in a random order, all of them from D = 6 on."""
    rng = np.random.default_rng(seed)
    reps = -(-D // len(POLES))
    return rng.permutation(np.tile(POLES, reps))[:D].copy() if D >= len(POLES) else rng.permutation(POLES)[:D].copy()


@functools.lru_cache(maxsize=None)
def case(D, T):
    """(x [D, T] float32, a [D] float64) of a test case: 3 N(0, 1) + 5, the last row with a step of 1e6 from T // 2 on;
    POLES in a random order, and from T = TILE - 1 on the first row takes the pole nearest 1, the hardest.  Cached and
    read-only."""
    rng = np.random.default_rng(7919 * D + T)
    x = (3.0 * rng.standard_normal((D, T)) + 5.0).astype(np.float32)
    if T >= 2:
        x[D - 1, T // 2 :] += np.float32(1e6)
    a = poles_of(D, 31 * D + T)
    if T >= TILE - 1:
        a[0] = POLES[-1]
    x.setflags(write=False), a.setflags(write=False)
    return x, a


@functools.lru_cache(maxsize=None)
def case_forward64(D, T, init):
    x, a = case(D, T)
    y = forward64(x, a, init)
    y.setflags(write=False)
    return y


def blocked_scan(x, a, init, carry_dtype=np.float64, drop_seam=None):
    """One row ``x`` [T] through the lag as a time-parallel kernel evaluates it, in float64: tiles of TILE samples, each
    run from a zero state (B), and y[t] = a^(k + 1) carry + B[k] with the carry of the previous tile -- kept in
    ``carry_dtype`` (np.float32: the mistake of a float32 carry) and dropped in front of tile ``drop_seam`` (the mistake of
    a lost carry).  Returns float64 [T], not rounded to float32."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    a = float(a)
    g = 1.0 - a
    T = x64.size
    y = np.empty(T)
    carry = 0.0
    for j0 in range(0, T, TILE):
        n = min(TILE, T - j0)
        B = np.empty(n)
        s = 0.0
        for k in range(n):
            s = x64[0] if (init and j0 + k == 0) else a * s + g * x64[j0 + k]
            B[k] = s
        if drop_seam is not None and j0 == drop_seam * TILE:
            carry = 0.0
        powers = a ** np.arange(1, n + 1, dtype=np.float64)
        if init and j0 == 0:
            powers[:] = 0.0  # (nothing in front of sample 0; the carry is 0 anyway)
        y[j0 : j0 + n] = powers * carry + B
        carry = float(carry_dtype(y[j0 + n - 1]))
    return y
