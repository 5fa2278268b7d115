"""Planar and quadratic sky subtraction across the focal plane (Sayers et al. 2010, for Bolocam): at every sample a
low-order polynomial in the detectors' focal-plane offsets is fitted across the detectors of a group and subtracted, on
the device, flagged samples left out of every sum (``mrx_tod_column_fit``, ``mrx_tod_column_apply``).  The
transpose of ``maria_amd.regress``: there the templates run along time and every detector has its coefficients, here
they run along the detectors and every sample has its own.

    term(d, t)  = float64(x[d, t]) - float64(model[d, t])
    r[g, i, t]  = sum over rows d of group g with v[d] > 0 and flags[d, t] == 0 of (u[d] * P[d, i]) * (term(d, t) - off[d])
    N[g, ij, t] = sum over the same rows of (v[d] * P[d, i]) * P[d, j], i <= j;   hits[g, t] = their number
    c[g, :, t]  = the solution of N c = r (scaled Cholesky, the verdict of ``regress.solve``), 0 where there is none
    y[d, t]     = x[d, t] + sign * float32(e[d] + h[d] * sum over i, in order, of c[g, i, t] * P[d, i])

``groups`` is one int32 entry per row, -1 for a row that takes part in nothing.  Every sum is added in the ascending row
order of the group, without atomics: the same inputs give the same bits on every call.  tests/skypoly_ref.py restates
everything in numpy."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_count, check_like, check_min_hits, check_out, check_sign, check_x, context, row_pitch

MAX_GROUPS = 16  # mrx_skypoly.hip: kMaxGroups
MAX_TERMS = 6    # mrx_skypoly.hip: kMaxTerms
MAX_ORDER = 2


def n_terms(order):
    """The terms of a two-dimensional polynomial of degree ``order``: 1, 3 or 6 for 0, 1 or 2."""
    if isinstance(order, bool) or int(order) != order or not 0 <= int(order) <= MAX_ORDER:
        raise ValueError(f"order {order}: 0 (a constant), 1 (a plane) or 2 (a quadratic surface)")
    order = int(order)
    return (order + 1) * (order + 2) // 2


def basis(offsets, order, groups=None, n_groups=1):
    """[D, K] float64: the terms 1, x, y, x^2, x y, y^2 (the first ``n_terms(order)`` of them) at the [D, 2] detector
    ``offsets``.  Per group x, y are the offsets less the group's mean, divided by the group's largest radius about that
    mean (1 where that is 0), so every term lies in [-1, 1].  A row outside every group gets zeros."""
    K = n_terms(order)
    off = np.asarray(offsets, np.float64)
    if off.ndim != 2 or off.shape[1] != 2 or off.shape[0] < 1 or not np.all(np.isfinite(off)):
        raise ValueError("offsets must be a finite [D, 2] array")
    D = off.shape[0]
    G = check_count(n_groups, "n_groups", MAX_GROUPS)
    if groups is None:
        gr = np.zeros(D, np.int64)
    else:
        gr = np.asarray(groups)
        if gr.ndim != 1 or gr.size != D or gr.dtype.kind not in "iu":
            raise ValueError(f"groups must be {D} integers, one per row")
        gr = gr.astype(np.int64)
    P = np.zeros((D, MAX_TERMS))
    for g in range(G):
        rows = gr == g
        if not rows.any():
            continue
        xy = off[rows] - off[rows].mean(axis=0)
        radius = np.sqrt((xy * xy).sum(axis=1)).max()
        xy = xy / (radius if radius > 0 else 1.0)
        x, y = xy[:, 0], xy[:, 1]
        P[rows] = np.stack([np.ones_like(x), x, y, x * x, x * y, y * y], axis=1)
    return np.ascontiguousarray(P[:, :K])


def _check_groups(groups, x, D):
    from .regress import _check_groups as check

    return check(groups, x, D)


def _check_f64(a, name, x, shape):
    import torch

    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or tuple(a.shape) != tuple(shape) or a.device != x.device:
        raise ValueError(f"{name} must be a {list(shape)} float64 tensor on x's device")
    return a.contiguous()


def _check_basis(P, x, D):
    import torch

    if not isinstance(P, torch.Tensor) or P.dim() != 2 or P.dtype != torch.float64 or P.shape[0] != D or P.device != x.device:
        raise ValueError(f"P must be a [{D}, K] float64 tensor on x's device")
    K = check_count(P.shape[1], "K", MAX_TERMS)
    return P.contiguous(), K


def fit(x, P, u, v, off=None, groups=None, n_groups=1, flags=None, model=None, min_hits=8, rcond=1e-10, sums=False, ctx=None):
    """``(c, ok, hits, N, r)`` of a [D, T] float32 device tensor ``x`` (any row pitch) against the basis ``P`` [D, K]
    float64 (K <= 6): the coefficients c [n_groups, K, T] float64 of every sample, ok [n_groups, T] bool (c is 0 where it
    is False), and with ``sums`` hits [n_groups, T] int64, N [n_groups, K (K + 1) / 2, T] and r [n_groups, K, T] float64
    (else None each); the formulas are at the top of the module.  ``u``, ``v``, ``off``: [D] float64 tensors (``off``
    None: zeros); a row with v <= 0 is not read.  ``min_hits`` (>= 1): the rows a sample needs, at least K.  Everything
    ``mrx_tod_column_fit`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    G = check_count(n_groups, "n_groups", MAX_GROUPS)
    P, K = _check_basis(P, x, D)
    u, v = _check_f64(u, "u", x, (D,)), _check_f64(v, "v", x, (D,))
    off = _check_f64(off, "off", x, (D,)) if off is not None else None
    groups = _check_groups(groups, x, D)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    min_hits = check_min_hits(min_hits, allow_bool=False)
    if min_hits < 1:
        raise ValueError(f"min_hits {min_hits}: an integer >= 1")
    if not 0.0 <= float(rcond) < 1.0:
        raise ValueError(f"rcond {rcond}: in [0, 1)")
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    dev = x.device
    c = torch.empty((G, K, T), dtype=torch.float64, device=dev)
    ok = torch.empty((G, T), dtype=torch.uint8, device=dev)
    hits = torch.empty((G, T), dtype=torch.int32, device=dev) if sums else None
    N = torch.empty((G, K * (K + 1) // 2, T), dtype=torch.float64, device=dev) if sums else None
    r = torch.empty((G, K, T), dtype=torch.float64, device=dev) if sums else None
    context(ctx, x).call("mrx_tod_column_fit", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(groups), G, ptr(P), K, ptr(u), ptr(v),
                         ptr(off), min_hits, float(rcond), ptr(c), T, ptr(ok), ptr(hits), ptr(N), ptr(r))
    return c, ok != 0, hits.to(torch.int64) if sums else None, N, r


def apply(x, P, c, h, e=None, groups=None, sign=-1, out=None, ctx=None):
    """y = x + sign * float32(e[d] + h[d] * sum_i c[g, i, t] * P[d, i]) (sign -1 or +1; rows of group -1 copied) of a
    [D, T] float32 device tensor ``x`` (any row pitch), the basis ``P`` [D, K] float64, coefficients ``c`` [G, K, T]
    float64 and ``h``, ``e`` [D] float64 (``e`` None: zeros); returns ``out`` (None: a new tensor; ``x`` itself: in
    place; otherwise a [D, T] float32 tensor of any row pitch that does not overlap x).  Everything
    ``mrx_tod_column_apply`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    P, K = _check_basis(P, x, D)
    if not isinstance(c, torch.Tensor) or c.dim() != 3:
        raise ValueError("c must be a [G, K, T] float64 tensor on x's device")
    G = check_count(c.shape[0], "the number of groups", MAX_GROUPS)
    c = _check_f64(c, "c", x, (G, K, T))
    h = _check_f64(h, "h", x, (D,))
    e = _check_f64(e, "e", x, (D,)) if e is not None else None
    groups = _check_groups(groups, x, D)
    sign = check_sign(sign)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    else:
        check_out(out, x, D, T, in_place=True)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    context(ctx, x).call("mrx_tod_column_apply", ptr(x), ld_x, D, T, ptr(groups), G, ptr(P), K, ptr(c), T, ptr(e), ptr(h), sign, ptr(out),
                         row_pitch(out))
    return out


def fit_sky(x, P, groups=None, n_groups=1, flags=None, model=None, n_iter=3, min_hits=8, min_dets=None, rcond=1e-10, ctx=None):
    """``(c, ok_t, gains, offsets, ok_d)``: every detector's gain g and offset o against its group's common mode and
    the verdict ok_d [D] from ``regress.fit_common_mode`` (``n_iter``, ``min_hits``, ``rcond``), unchanged; then ONE
    ``fit`` with u = w g, v = (w g) g, off = o, w = ok_d: at every sample the gain-weighted least-squares surface
    sum_k c_k(t) P_dk through (x - o_d) / g_d.  c [G, K, T] float64 and ok_t [G, T] bool; ``min_dets`` (None: 2 K): the
    detectors a sample needs.  A detector with ok_d False takes no part."""
    import torch

    from . import regress

    if not isinstance(P, torch.Tensor) or P.dim() != 2:
        raise ValueError("P must be a [D, K] float64 tensor on x's device")
    K = check_count(P.shape[1], "K", MAX_TERMS)
    min_dets = 2 * K if min_dets is None else min_dets
    if isinstance(min_dets, bool) or int(min_dets) != min_dets or int(min_dets) < 1:
        raise ValueError(f"min_dets {min_dets}: None or an integer >= 1")
    ctx_ = None if not isinstance(x, torch.Tensor) or not x.is_cuda else context(ctx, x)
    _, a, g, ok_d, _ = regress.fit_common_mode(x, groups=groups, n_groups=n_groups, flags=flags, model=model, n_iter=n_iter, min_hits=min_hits,
                                               rcond=rcond, ctx=ctx_)
    w = ok_d.to(torch.float64)
    g = torch.where(ok_d, g, torch.zeros_like(g))
    o = torch.where(ok_d, a[:, 0], torch.zeros_like(g)).contiguous()
    c, ok_t, _, _, _ = fit(x, P, w * g, (w * g) * g, off=o, groups=groups, n_groups=n_groups, flags=flags, model=model, min_hits=int(min_dets),
                           rcond=rcond, ctx=ctx_)
    return c, ok_t, g, o, ok_d


def inject_gradient(x, P, c, gains=None, offsets=None, groups=None, out=None, ctx=None):
    """x + float32(offsets[d] + gains[d] * sum_k c[g, k, t] * P[d, k]): test data with a known surface drifting across the
    focal plane, put in with ``apply(sign=+1)`` (``gains`` None: ones; ``offsets`` None: zeros)."""
    import torch

    D = check_x(x)[0]
    h = torch.ones(D, dtype=torch.float64, device=x.device) if gains is None else gains
    return apply(x, P, c, h, e=offsets, groups=groups, sign=+1, out=out, ctx=ctx)
