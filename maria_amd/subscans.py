"""The subscan polynomial filter: a constant-elevation scan, its segmentation at the turnarounds, and a Legendre fit per
(detector, segment) on the device, flagged samples left out of every sum (``mrx_tod_segment_normal``,
``mrx_tod_segment_apply``).

``bounds`` [S + 1] int32, ascending, cuts a row of T samples into S segments [bounds[s], bounds[s + 1]) (clamped to
0 .. T; an empty one is allowed; samples before bounds[0] or from bounds[S] on belong to nothing).  In a segment [lo, hi)
of L samples:

    u(t)          = (2 (t - lo) - (L - 1)) / (L - 1)   (0 where L = 1): lo -> -1, hi - 1 -> +1
    P_0 = 1, P_1 = u, P_{n+1} = ((2 n + 1) u P_n - n P_{n-1}) / (n + 1)               (Legendre, Bonnet's recursion)
    term(d, t)    = float64(x[d, t]) - float64(model[d, t])
    N[d, s, i, j] = sum over the segment's t with flags[d, t] == 0 of P_i P_j;   r[d, s, i] = of P_i term(d, t)
    y[d, t]       = x[d, t] + sign * float32(sum over i, in order, of a[d, s, i] P_i)

The polynomials are evaluated in the kernels, in float64, and never stored.  Every sum is added in a fixed order (a
function of the segment's ends alone), without atomics: the same inputs give the same bits on every call.  The order of
the operations is written out in include/mrx.h, and tests/subscans_ref.py restates it in numpy.

With the flags fixed the filter is a linear operator, F = I - T A T^t M (M = (flags == 0), T the basis, A = N^-1 where the
pair can be fitted and 0 otherwise): ``freeze`` gives A, ``project`` applies F or F^t in one fused pass
(``mrx_tod_segment_project``), and ``Projector`` holds both for one TOD, for ``MaximumLikelihoodMapper(subscan_filter=...)``
(tests/subscan_project_ref.py restates it in numpy)."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_count, check_like, check_min_hits, check_out, check_sign, check_x, context, row_pitch
from .regress import MAX_TEMPLATES, solve

MAX_ORDER = MAX_TEMPLATES  # mrx_subscan.hip: kMaxOrder, the number K of polynomials P_0 .. P_{K - 1}


def back_and_forth(t, throw, speed, accel):
    """The azimuth offset x(t) of a constant-elevation sweep, in the units of ``throw``: constant ``speed`` across
    -throw .. +throw, turnarounds at constant ``accel`` beyond them.  With tc = 2 throw / speed (a crossing),
    tt = 2 speed / accel (a turnaround), the period 2 (tc + tt) and tau = t mod (tc + tt):

        x = -throw + speed tau                                   for tau < tc
        x = +throw + speed (tau - tc) - accel (tau - tc)^2 / 2   for tau >= tc    (overshoot speed^2 / (2 accel))

    with the sign of x reversed in every second half period.  It starts at -throw moving up."""
    t = np.asarray(t, np.float64)
    throw, speed, accel = float(throw), float(speed), float(accel)
    if not (np.isfinite(throw) and np.isfinite(speed) and np.isfinite(accel) and throw > 0 and speed > 0 and accel > 0):
        raise ValueError(f"throw {throw}, speed {speed}, accel {accel}: three finite numbers > 0")
    tc, tt = 2.0 * throw / speed, 2.0 * speed / accel
    half = tc + tt
    k = np.floor(t / half)
    tau = t - k * half
    w = tau - tc
    x = np.where(tau < tc, -throw + speed * tau, throw + speed * w - 0.5 * accel * w * w)
    return np.where(k % 2 == 0, x, -x)


def find_subscans(az, turn_frac=0.9):
    """``(bounds int32 [S + 1], turn uint8 [T])`` of a boresight azimuth ``az`` [T] (radians; unwrapped here).  With
    v[t] = az[t + 1] - az[t] (the last value repeated), zeros taking the sign before them and leading zeros the first
    nonzero sign: a segment starts at every t whose sign differs from that of t - 1, bounds = [0, cuts.., T], and
    turn[t] = |v[t]| < turn_frac median|v|.  T < 2 or a constant azimuth: one segment, no turnaround."""
    az = np.asarray(az, np.float64)
    if az.ndim != 1 or az.size < 1 or not np.all(np.isfinite(az)):
        raise ValueError("az must be a one-dimensional array of T >= 1 finite angles")
    if not 0.0 <= float(turn_frac) <= 1.0:
        raise ValueError(f"turn_frac {turn_frac}: in [0, 1]")
    T = az.size
    if T < 2:
        return np.array([0, T], np.int32), np.zeros(T, np.uint8)
    v = np.diff(np.unwrap(az))
    v = np.append(v, v[-1])
    sign = np.sign(v).astype(np.int64)
    moving = np.flatnonzero(sign)
    if moving.size == 0:
        return np.array([0, T], np.int32), np.zeros(T, np.uint8)
    last = np.maximum.accumulate(np.where(sign != 0, np.arange(T), -1))  # the last moving sample at or before t
    sign = sign[np.where(last >= 0, last, moving[0])]
    cuts = np.flatnonzero(sign[1:] != sign[:-1]) + 1
    bounds = np.concatenate([[0], cuts, [T]]).astype(np.int32)
    turn = (np.abs(v) < float(turn_frac) * np.median(np.abs(v))).astype(np.uint8)
    return bounds, turn


def _check_bounds(bounds, x):
    """(the [S + 1] int32 tensor on x's device, S) of ``bounds``: integers, one-dimensional, at least two, ascending."""
    import torch

    if isinstance(bounds, torch.Tensor):
        if bounds.dtype not in (torch.int32, torch.int64):
            raise ValueError("bounds must be integers")
        b = bounds.detach().cpu().numpy()
    else:
        b = np.asarray(bounds)
    if b.ndim != 1 or b.size < 2 or b.dtype.kind not in "iu":
        raise ValueError("bounds must be a one-dimensional array of S + 1 >= 2 integers")
    b = b.astype(np.int64)
    if np.any(np.diff(b) < 0) or b.min() < np.iinfo(np.int32).min or b.max() > np.iinfo(np.int32).max:
        raise ValueError("bounds must ascend (equal neighbours: an empty segment) and fit int32")
    if isinstance(bounds, torch.Tensor) and bounds.dtype == torch.int32 and bounds.device == x.device and bounds.is_contiguous():
        return bounds, b.size - 1
    return torch.as_tensor(b.astype(np.int32)).to(x.device), b.size - 1


def _check_coefficients(a, x, D, S):
    import torch

    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or a.dim() != 3 or tuple(a.shape[:2]) != (D, S) or a.device != x.device:
        raise ValueError(f"a must be a [{D}, {S}, K] float64 tensor on x's device")
    return a.contiguous(), check_count(a.shape[2], "K", MAX_ORDER)


def normal_equations(x, bounds, K, flags=None, model=None, ctx=None):
    """``(N, r, hits)`` of every (row, segment) of ``x`` ([D, T] float32 device tensor, any row pitch) against
    P_0 .. P_{K - 1} (K <= 8): [D, S, K, K] float64, [D, S, K] float64 and [D, S] int64 device tensors; an empty segment
    gets zeros.  ``flags`` [D, T] uint8 and ``model`` [D, T] float32, any row pitch.  Everything
    ``mrx_tod_segment_normal`` refuses, and bounds that do not ascend, raise ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    K = check_count(K, "K", MAX_ORDER)
    d_bounds, S = _check_bounds(bounds, x)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    N = torch.empty((D, S, K, K), dtype=torch.float64, device=x.device)
    r = torch.empty((D, S, K), dtype=torch.float64, device=x.device)
    hits = torch.empty((D, S), dtype=torch.int32, device=x.device)
    context(ctx, x).call("mrx_tod_segment_normal", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(d_bounds), S, K, ptr(N), ptr(r),
                         ptr(hits))
    return N, r, hits.to(torch.int64)


def fit(x, bounds, K, flags=None, model=None, min_hits=8, rcond=1e-10, ctx=None):
    """``(a [D, S, K] float64, ok [D, S] bool)``: every (row, segment)'s least-squares coefficients of P_0 .. P_{K - 1},
    ``regress.solve`` of ``normal_equations`` on their [D S, ..] views with its ``min_hits`` and ``rcond``: a pair that is
    not ok (fewer than max(min_hits, K) samples kept, or polynomials degenerate on them) gets a = 0.  No host
    synchronisation once ``bounds`` is on the device."""
    min_hits = check_min_hits(min_hits)
    if not 0.0 <= float(rcond) < 1.0:
        raise ValueError(f"rcond {rcond}: in [0, 1)")
    N, r, hits = normal_equations(x, bounds, K, flags=flags, model=model, ctx=ctx)
    D, S, K = r.shape
    a, ok = solve(N.view(D * S, K, K), r.view(D * S, K), hits.view(D * S), min_hits=min_hits, rcond=rcond)
    return a.view(D, S, K), ok.view(D, S)


def apply(x, bounds, a, sign=-1, out=None, ctx=None):
    """y = x + sign * float32(sum_i a[d, s, i] P_i) (sign -1 or +1) of a [D, T] float32 device tensor ``x`` (any row
    pitch) and coefficients ``a`` [D, S, K] float64; samples in no segment are copied.  Returns ``out`` (None: a new
    tensor; ``x`` itself: in place; otherwise a [D, T] float32 tensor of any row pitch that does not overlap x).
    Everything ``mrx_tod_segment_apply`` refuses, and bounds that do not ascend, raise ValueError before any device
    call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    d_bounds, S = _check_bounds(bounds, x)
    a, K = _check_coefficients(a, x, D, S)
    sign = check_sign(sign)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    else:
        check_out(out, x, D, T, in_place=True)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    context(ctx, x).call("mrx_tod_segment_apply", ptr(x), ld_x, D, T, ptr(d_bounds), S, K, ptr(a), sign, ptr(out), row_pitch(out))
    return out


def inject_drifts(x, bounds, coeffs, ctx=None):
    """A new tensor: ``x`` plus the polynomial drifts ``coeffs`` [D, S, K] float64, ``apply`` with sign +1 (for tests and
    demonstrations)."""
    return apply(x, bounds, coeffs, sign=+1, ctx=ctx)


def freeze(N, hits, min_hits=8, rcond=1e-10):
    """``(A [D, S, K, K] float64, ok [D, S] uint8)``: the inverse of every (row, segment)'s normal matrix, for ``project``.
    ``ok`` is ``regress.solve``'s verdict on the same N, hits, ``min_hits`` and ``rcond``; with its scaled Cholesky factor
    L of M = (N * s_i) * s_j, s = 1 / sqrt(diag N):  B = (cholesky_solve(I, L) * s_i) * s_j,  A = (B + B^T) / 2 (the same
    bits on both sides of the diagonal, a + b being b + a), and zero where the pair is not ok.  N does not depend on the
    data: ``normal_equations`` of any [D, T] buffer under the flags gives it.  On the tensors' device, no host
    synchronisation."""
    import torch

    from .regress import scaled_factor

    if not isinstance(N, torch.Tensor) or N.dim() != 4 or N.shape[2] != N.shape[3] or N.dtype != torch.float64:
        raise ValueError("N must be a [D, S, K, K] float64 tensor")
    D, S, K = N.shape[:3]
    if not isinstance(hits, torch.Tensor) or tuple(hits.shape) != (D, S) or hits.dtype.is_floating_point or hits.device != N.device:
        raise ValueError(f"hits must be a [{D}, {S}] integer tensor on N's device")
    L, s, ok = scaled_factor(N.reshape(D * S, K, K), hits.reshape(D * S), min_hits, rcond)
    eye = torch.eye(K, dtype=torch.float64, device=N.device).expand(D * S, K, K)
    B = (torch.cholesky_solve(eye, L) * s[:, :, None]) * s[:, None, :]
    A = (B + B.transpose(1, 2)) * 0.5
    A = torch.where(ok[:, None, None], A, torch.zeros_like(A))
    return A.view(D, S, K, K).contiguous(), ok.view(D, S).to(torch.uint8)


def project(x, bounds, A, ok, flags=None, transpose=False, coefficients=False, ctx=None):
    """The frozen subscan filter on ``x`` ([D, T] float32 device tensor, any row pitch), in place: with M = (flags == 0),
    T the segment's basis and ``A``, ``ok`` of ``freeze``,  x <- F x = x - T A T^t M x,  or with ``transpose``
    x <- F^t x = x - M T A T^t x  (``mrx_tod_segment_project``; the order of every sum is in include/mrx.h).  A pair that
    is not ok and samples in no segment keep their bits.  Returns ``x``, or with ``coefficients`` ``(x, a [D, S, K]
    float64)``, a = A T^t M x (A T^t x transposed).  Everything the entry refuses, and bounds that do not ascend, raise
    ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    d_bounds, S = _check_bounds(bounds, x)
    if not isinstance(A, torch.Tensor) or A.dtype != torch.float64 or A.dim() != 4 or tuple(A.shape[:2]) != (D, S) or A.shape[2] != A.shape[3] \
            or A.device != x.device:
        raise ValueError(f"A must be a [{D}, {S}, K, K] float64 tensor on x's device")
    K = check_count(A.shape[2], "K", MAX_ORDER)
    if not isinstance(ok, torch.Tensor) or ok.dtype not in (torch.uint8, torch.bool) or tuple(ok.shape) != (D, S) or ok.device != x.device:
        raise ValueError(f"ok must be a [{D}, {S}] uint8 tensor on x's device")
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    if not isinstance(transpose, (bool, np.bool_)):
        raise ValueError(f"transpose {transpose!r}: True or False")
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    A, ok = A.contiguous(), ok.to(torch.uint8).contiguous()
    a = torch.empty((D, S, K), dtype=torch.float64, device=x.device) if coefficients else None
    context(ctx, x).call("mrx_tod_segment_project", ptr(x), ld_x, ptr(flags), ld_f, D, T, ptr(d_bounds), S, K, ptr(A), ptr(ok), int(bool(transpose)),
                         ptr(a))
    return (x, a) if coefficients else x


class Projector:
    """The subscan filter of one TOD as a fixed linear operator F' on float32 [D, T] device tensors, in place:
    ``bounds`` [S + 1], ``K`` polynomials, ``flags`` ([D, T] uint8 device tensor or None) and, frozen from them alone,
    ``A`` and ``ok`` (``freeze`` of ``normal_equations`` of ``like``, any [D, T] float32 device tensor: N does not depend
    on the data).  F' T = 0 under its own mask, so F' F = F' for any earlier subscan filter F on these segments and this
    order: a mapper needs nothing of that filter's state."""

    def __init__(self, like, bounds, K, flags=None, min_hits=8, rcond=1e-10, ctx=None):
        min_hits = check_min_hits(min_hits)
        if not 0.0 <= float(rcond) < 1.0:
            raise ValueError(f"rcond {rcond}: in [0, 1)")
        N, _, hits = normal_equations(like, bounds, K, flags=flags, ctx=ctx)
        self.bounds, self.K, self.flags, self.ctx, self.T = _check_bounds(bounds, like)[0], int(K), flags, ctx, int(like.shape[1])
        self.A, self.ok = freeze(N, hits, min_hits=min_hits, rcond=rcond)

    def apply(self, buf):
        """buf <- F' buf."""
        return project(buf, self.bounds, self.A, self.ok, flags=self.flags, ctx=self.ctx)

    def apply_transpose(self, buf):
        """buf <- F'^t buf."""
        return project(buf, self.bounds, self.A, self.ok, flags=self.flags, transpose=True, ctx=self.ctx)

    def product(self):
        """What a mapper reports: ``order``, ``bounds`` and ``unfitted``, the [n, 2] (detector, segment) pairs of the
        segments with samples on which F' is the identity (numpy)."""
        bounds = self.bounds.cpu().numpy()
        nonempty = np.diff(np.clip(bounds.astype(np.int64), 0, self.T)) > 0
        return {"order": self.K - 1, "bounds": bounds, "unfitted": np.argwhere((self.ok.cpu().numpy() == 0) & nonempty[None, :])}
