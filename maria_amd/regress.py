"""The common mode of a [D, T] TOD and other time templates shared by detectors, fitted per detector and removed on the
device, flagged samples left out of every sum (``mrx_tod_column_mean``, ``mrx_tod_regress_normal``,
``mrx_tod_regress_apply``).

    term(d, t)  = float64(x[d, t]) - float64(model[d, t])
    S[g, t]     = sum over rows d of group g with flags[d, t] == 0 of u[d] * (term(d, t) - off[d]);  W[g, t] = sum of v[d]
    mean[g, t]  = float32(S / W) where W > 0, else 0
    N[d, i, j]  = sum over t with flags[d, t] == 0 of float64(B[g, i, t]) * float64(B[g, j, t])
    r[d, i]     = sum over the same t of float64(B[g, i, t]) * term(d, t);   hits[d] = their number
    y[d, t]     = x[d, t] + sign * float32(sum over i, in order, of a[d, i] * float64(B[g, i, t]))

``groups`` is one int32 entry per row, -1 for a row that takes part in nothing.  Every float64 sum is added in a fixed
order (rows: ascending within the group; time: a function of T alone), without atomics: the same inputs give the same
bits on every call.  ``fit_common_mode`` iterates mean and fit; its steps are written out in its docstring, and
tests/regress_ref.py restates them in numpy."""

from __future__ import annotations

import numpy as np

from ._tod_args import check_count, check_like, check_min_hits, check_out, check_sign, check_x, context, row_pitch

MAX_GROUPS = 16    # mrx_regress.hip: kMaxGroups
MAX_TEMPLATES = 8  # mrx_regress.hip: kMaxTemplates


def _check_groups(groups, x, D):
    """None, or the [D] int32 tensor on x's device of ``groups`` (a tensor or an integer array)."""
    import torch

    if groups is None:
        return None
    if isinstance(groups, torch.Tensor):
        if groups.dim() != 1 or groups.shape[0] != D or groups.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"groups must be {D} integers, one per row")
        return groups.to(x.device, torch.int32).contiguous()
    g = np.asarray(groups)
    if g.ndim != 1 or g.size != D or g.dtype.kind not in "iu":
        raise ValueError(f"groups must be {D} integers, one per row")
    return torch.as_tensor(np.ascontiguousarray(g, np.int32)).to(x.device)


def _check_vector(a, name, x, D, K=None):
    import torch

    shape = (D,) if K is None else (D, K)
    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or tuple(a.shape) != shape or a.device != x.device:
        raise ValueError(f"{name} must be a {list(shape)} float64 tensor on x's device")
    return a.contiguous()


def _check_templates(B, x, G, T):
    """(K, pitch) of the [G, K, T] float32 templates: unit stride along time, pitch >= T, rows and groups evenly spaced."""
    import torch

    if not isinstance(B, torch.Tensor) or B.dim() != 3 or B.dtype != torch.float32 or B.shape[0] != G or B.shape[2] != T or B.device != x.device:
        raise ValueError(f"B must be a [{G}, K, {T}] float32 tensor on x's device")
    K = check_count(B.shape[1], "K", MAX_TEMPLATES)
    ld = B.stride(1) if K > 1 else (B.stride(0) if G > 1 else T)
    if (T > 1 and B.stride(2) != 1) or ld < T or (G > 1 and B.stride(0) != K * ld):
        raise ValueError("B must have unit stride along time and one row pitch >= T for all of its G * K rows")
    return K, ld


def column_mean(x, u, v, off=None, groups=None, n_groups=1, flags=None, model=None, ctx=None):
    """``(mean, S, W)`` of a [D, T] float32 device tensor ``x`` (any row pitch): [n_groups, T] device tensors, float32,
    float64 and float64 (the formulas are at the top of the module).  ``u``, ``v``, ``off``: [D] float64 tensors
    (``off`` None: zeros); ``groups``: [D] integers (None: all rows in group 0); ``flags`` [D, T] uint8 and ``model``
    [D, T] float32, any row pitch.  Everything ``mrx_tod_column_mean`` refuses raises ValueError before any device
    call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    G = check_count(n_groups, "n_groups", MAX_GROUPS)
    u, v = _check_vector(u, "u", x, D), _check_vector(v, "v", x, D)
    off = _check_vector(off, "off", x, D) if off is not None else None
    groups = _check_groups(groups, x, D)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    if not x.is_cuda:  # the last refusal: a host tensor gets every other one first
        raise ValueError("x must be a device tensor")
    S = torch.empty((G, T), dtype=torch.float64, device=x.device)
    W = torch.empty((G, T), dtype=torch.float64, device=x.device)
    mean = torch.empty((G, T), dtype=torch.float32, device=x.device)
    context(ctx, x).call("mrx_tod_column_mean", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(groups), G, ptr(u), ptr(v),
                         ptr(off), ptr(S), ptr(W), ptr(mean), T)
    return mean, S, W


def normal_equations(x, B, groups=None, flags=None, model=None, ctx=None):
    """``(N, r, hits)`` of every row of ``x`` ([D, T] float32 device tensor, any row pitch) against the templates of its
    group, ``B`` [G, K, T] float32 (K <= 8, G <= 16): [D, K, K] float64, [D, K] float64 and [D] int64 device tensors.  A
    row of group -1 gets zeros.  Everything ``mrx_tod_regress_normal`` refuses raises ValueError before any device
    call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    if not isinstance(B, torch.Tensor) or B.dim() != 3:
        raise ValueError("B must be a [G, K, T] float32 tensor on x's device")
    G = check_count(B.shape[0], "the number of groups", MAX_GROUPS)
    K, ld_b = _check_templates(B, x, G, T)
    groups = _check_groups(groups, x, D)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    N = torch.empty((D, K, K), dtype=torch.float64, device=x.device)
    r = torch.empty((D, K), dtype=torch.float64, device=x.device)
    hits = torch.empty((D,), dtype=torch.int32, device=x.device)
    context(ctx, x).call("mrx_tod_regress_normal", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, D, T, ptr(groups), G, ptr(B), ld_b, K,
                         ptr(N), ptr(r), ptr(hits))
    return N, r, hits.to(torch.int64)


def apply(x, B, a, groups=None, sign=-1, out=None, ctx=None):
    """y = x + sign * float32(sum_i a[d, i] * B[g, i, t]) (sign -1 or +1; rows of group -1 copied) of a [D, T] float32
    device tensor ``x`` (any row pitch), templates ``B`` [G, K, T] float32 and coefficients ``a`` [D, K] float64; returns
    ``out`` (None: a new tensor; ``x`` itself: in place; otherwise a [D, T] float32 tensor of any row pitch that does not
    overlap x).  Everything ``mrx_tod_regress_apply`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    if not isinstance(B, torch.Tensor) or B.dim() != 3:
        raise ValueError("B must be a [G, K, T] float32 tensor on x's device")
    G = check_count(B.shape[0], "the number of groups", MAX_GROUPS)
    K, ld_b = _check_templates(B, x, G, T)
    a = _check_vector(a, "a", x, D, K)
    groups = _check_groups(groups, x, D)
    sign = check_sign(sign)
    if out is None:
        out = torch.empty((D, T), dtype=torch.float32, device=x.device)
    else:
        check_out(out, x, D, T, in_place=True)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    context(ctx, x).call("mrx_tod_regress_apply", ptr(x), ld_x, D, T, ptr(groups), G, ptr(B), ld_b, K, ptr(a), sign, ptr(out),
                         row_pitch(out))
    return out


def solve(N, r, hits, min_hits=8, rcond=1e-10):
    """``(a [D, K] float64, ok [D] bool)``: the solutions of N[d] a[d] = r[d], in float64 with torch on the tensors' device,
    without a host synchronisation.  With s = 1 / sqrt(diag N), M = (N * s_i) * s_j and L the Cholesky factor of M
    (``torch.linalg.cholesky_ex``): a = s * cholesky_solve(s * r, L).  A row is not ok, and gets a = 0, when
    hits < max(min_hits, K), a diagonal entry of N is not > 0, the factorisation reports failure, or the smallest pivot
    of M, min_i L_ii^2 (the share of template i that is orthogonal to the templates before it), is below ``rcond``."""
    import torch

    if not isinstance(N, torch.Tensor) or not isinstance(r, torch.Tensor) or N.dim() != 3 or N.shape[1] != N.shape[2] or r.dim() != 2 \
            or N.shape[:2] != r.shape or N.dtype != torch.float64 or r.dtype != torch.float64:
        raise ValueError("N must be a [D, K, K] and r a [D, K] float64 tensor")
    L, s, ok = scaled_factor(N, hits, min_hits, rcond)
    a = torch.cholesky_solve((r * s)[:, :, None], L)[:, :, 0] * s
    return torch.where(ok[:, None], a, torch.zeros_like(a)), ok


def scaled_factor(N, hits, min_hits=8, rcond=1e-10):
    """``(L [D, K, K], s [D, K], ok [D] bool)`` of ``solve``: the Cholesky factor of M = (N * s_i) * s_j (the identity where
    the row is not ok), s = 1 / sqrt(diag N) and the verdict, for ``solve`` and for what freezes N^-1
    (``subscans.freeze``)."""
    import torch

    if not isinstance(N, torch.Tensor) or N.dim() != 3 or N.shape[1] != N.shape[2] or N.dtype != torch.float64:
        raise ValueError("N must be a [D, K, K] float64 tensor")
    D, K = N.shape[:2]
    check_count(K, "K", MAX_TEMPLATES)
    if not isinstance(hits, torch.Tensor) or tuple(hits.shape) != (D,) or hits.dtype.is_floating_point:
        raise ValueError(f"hits must be {D} integers, one per row")
    floor = max(check_min_hits(min_hits), K)
    if not 0.0 <= float(rcond) < 1.0:
        raise ValueError(f"rcond {rcond}: in [0, 1)")
    diag = torch.diagonal(N, dim1=1, dim2=2)
    good = (diag > 0).all(dim=1) & (hits >= floor)
    s = torch.where(diag > 0, diag, torch.ones_like(diag)).sqrt().reciprocal()
    eye = torch.eye(K, dtype=torch.float64, device=N.device).expand(D, K, K)
    M = torch.where(good[:, None, None], (N * s[:, :, None]) * s[:, None, :], eye)
    L, info = torch.linalg.cholesky_ex(M)
    pivot = torch.diagonal(L, dim1=1, dim2=2).square().amin(dim=1)
    ok = good & (info == 0) & (pivot >= float(rcond))  # a NaN pivot compares false
    return torch.where(ok[:, None, None], L, eye), s, ok


def legendre_templates(T, order):
    """[order + 1, T] float32: the Legendre polynomials P_0 .. P_order on ``linspace(-1, 1, T)``, by Bonnet's
    recursion (n + 1) P_{n+1} = (2 n + 1) x P_n - n P_{n-1} in float64."""
    if int(T) != T or int(T) < 1:
        raise ValueError(f"T {T}: an integer >= 1")
    if int(order) != order or not 0 <= int(order) < MAX_TEMPLATES:
        raise ValueError(f"order {order}: an integer in 0 .. {MAX_TEMPLATES - 1}")
    T, order = int(T), int(order)
    t = np.linspace(-1.0, 1.0, T)
    P = np.empty((order + 1, T))
    P[0] = 1.0
    if order >= 1:
        P[1] = t
    for n in range(1, order):
        P[n + 1] = ((2 * n + 1) * t * P[n] - n * P[n - 1]) / (n + 1)
    return P.astype(np.float32)


def airmass_template(el):
    """[T] float32: the plane-parallel airmass 1 / sin(el) of the boresight elevation ``el`` (radians, ``coords._bel``) less
    its mean, in float64."""
    el = np.asarray(el, np.float64)
    if el.ndim != 1 or el.size < 1 or not np.all(np.isfinite(el)) or np.any(el <= 0) or np.any(el > np.pi / 2 + 1e-9):
        raise ValueError("el must be a one-dimensional array of elevations in (0, pi / 2]")
    a = 1.0 / np.sin(el)
    return (a - a.mean()).astype(np.float32)


def _group_mean(w, val, onehot):
    """[G] float64: sum_d w val / sum_d w over each group's rows (``onehot`` [G, D]); 1 where the group has no weight or
    the mean is 0.  Plain torch sums: the same bits on every call."""
    import torch

    num = (onehot * (w * val)[None, :]).sum(dim=1)
    den = (onehot * w[None, :]).sum(dim=1)
    s = num / torch.where(den > 0, den, torch.ones_like(den))
    return torch.where((den > 0) & (s != 0), s, torch.ones_like(s))


def fit_common_mode(x, groups=None, n_groups=1, flags=None, model=None, extra=None, n_iter=3, min_hits=8, rcond=1e-10, ctx=None):
    """The common mode of each group of rows of ``x`` ([D, T] float32 device tensor) and every row's fit to it:
    ``(c, a, gains, ok, B)`` with c [G, T] float32, a [D, K] float64 (K = 2 + Ke: offset, gain on c, then ``extra``),
    gains [D] float64 (a[:, 1] over its group's weighted mean), ok [D] bool and B [G, K, T] float32, B[g] = [1, c_g,
    extra...].  ``extra``: a [Ke, T] float32 array or tensor of further templates shared by all groups, 2 + Ke <= 8.

    Start: grouped = groups inside 0 .. G - 1; (N, r, hits) = normal_equations against the constant alone;
    fit = hits >= max(min_hits, 1); o = r / hits where fit, else 0; w = 1 where grouped and fit, else 0; g = 1.
    Each of the ``n_iter`` iterations:
      1. c = column_mean(u = w g, v = (w g) g, off = o), as float32;
      2. B[g] = [1, c_g, extra...]; (N, r, hits) = normal_equations; (a, ok) = solve(N, r, hits, min_hits, rcond);
      3. o = a[:, 0]; w = 0 where not ok;
      4. s_g = sum w a[:, 1] / sum w over the group (1 for a group without weight or with s_g = 0); g = a[:, 1] / s_g.
    The coefficients of the last fit are the result; c is not recomputed after it.  No host synchronisation."""
    import torch

    D, T, _ = check_x(x)
    G = check_count(n_groups, "n_groups", MAX_GROUPS)
    n_iter = check_count(n_iter, "n_iter", 64)
    min_hits = check_min_hits(min_hits)
    if extra is not None:
        extra = extra if isinstance(extra, torch.Tensor) else torch.as_tensor(np.asarray(extra))
        if extra.dim() != 2 or extra.shape[1] != T or extra.dtype != torch.float32 or not 2 + extra.shape[0] <= MAX_TEMPLATES:
            raise ValueError(f"extra must be a [Ke, {T}] float32 array with 2 + Ke <= {MAX_TEMPLATES}")
    Ke = 0 if extra is None else int(extra.shape[0])
    d_groups = _check_groups(groups, x, D)
    if flags is not None:
        check_like(flags, "flags", x, D, T, "uint8")
    if model is not None:
        check_like(model, "model", x, D, T)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    ctx = context(ctx, x)
    dev = x.device
    idx = torch.zeros(D, dtype=torch.int64, device=dev) if d_groups is None else d_groups.to(torch.int64)
    grouped = (idx >= 0) & (idx < G)
    idx = torch.where(grouped, idx, torch.zeros_like(idx))
    onehot = ((torch.arange(G, device=dev)[:, None] == idx[None, :]) & grouped[None, :]).to(torch.float64)
    B = torch.ones((G, 2 + Ke, T), dtype=torch.float32, device=dev)
    if Ke:
        B[:, 2:, :] = extra.to(dev)[None]
    _, r, hits = normal_equations(x, B[:, :1, :], groups=d_groups, flags=flags, model=model, ctx=ctx)
    fit = hits >= max(min_hits, 1)
    o = torch.where(fit, r[:, 0] / torch.where(fit, hits, torch.ones_like(hits)).to(torch.float64), torch.zeros_like(r[:, 0]))
    w = (grouped & fit).to(torch.float64)
    g = torch.ones(D, dtype=torch.float64, device=dev)
    for _ in range(n_iter):
        c, _, _ = column_mean(x, w * g, (w * g) * g, off=o, groups=d_groups, n_groups=G, flags=flags, model=model, ctx=ctx)
        B[:, 1, :] = c
        N, r, hits = normal_equations(x, B, groups=d_groups, flags=flags, model=model, ctx=ctx)
        a, ok = solve(N, r, hits, min_hits=min_hits, rcond=rcond)
        o = a[:, 0].contiguous()
        w = torch.where(ok, w, torch.zeros_like(w))
        g = a[:, 1] / _group_mean(w, a[:, 1], onehot)[idx]
    return c, a, g, ok, B
