"""The TOD pre-processing F of maria_amd.tod_processing as a float64 numpy operator and its transpose,
step by step from the formulas, for the filter-aware map's tests.  ``build`` turns a process_tod config into a list of
steps; ``apply`` runs them in process_tod's order, ``apply_transpose`` their transposes in reverse order."""

import numpy as np
import scipy.signal


def line_weights(T):
    """(a, b): np.linspace(x_0, x_{T-1}, T)[t] = a_t x_0 + b_t x_{T-1} (T = 1: the line is x_0 itself)."""
    b = np.arange(T) / (T - 1) if T > 1 else np.ones(1)
    return 1.0 - b, b


def slope(x):
    """S x = x - (x_0 (1 - t/(T-1)) + x_{T-1} t/(T-1))."""
    a, b = line_weights(x.shape[1])
    return x - (x[:, :1] * a + x[:, -1:] * b)


def slope_transpose(u):
    """S^T u = u - e_0 sum_t (1 - t/(T-1)) u_t - e_{T-1} sum_t t/(T-1) u_t."""
    a, b = line_weights(u.shape[1])
    out = u.copy()
    out[:, 0] -= u @ a
    out[:, -1] -= u @ b
    return out


def build(config, t, el=None, modes=None):
    """The steps of ``config`` for a TOD with sample times ``t`` (and boresight elevation ``el``, for the spline's
    elevation gradient); ``modes`` = (U [D, m], n [D]) freezes remove_modes."""
    from maria_amd import tod_processing as tp

    t = np.asarray(t, float)
    T = t.size
    fs = 1.0 / np.mean(np.diff(t)) if T > 1 else 1.0
    steps = []
    if "remove_slope" in config:
        steps.append(("remove_slope", None))
    if "remove_spline" in config:
        sub = dict(config["remove_spline"])
        B = tp.bspline_basis(t, spacing=sub["knot_spacing"], order=sub.get("order", 3))
        if sub.get("remove_el_gradient", False) and "remove_el_gradient_order" not in sub:
            sub["remove_el_gradient_order"] = 2
        if "remove_el_gradient_order" in sub:
            rel = (np.asarray(el, float) - np.min(el)) / np.ptp(el)
            B = np.concatenate([B * rel**i for i in range(sub["remove_el_gradient_order"] + 1)], axis=0)
        steps.append(("remove_spline", (B, np.linalg.inv(B @ B.T) @ B)))
    if "window" in config:
        steps.append(("window", getattr(scipy.signal.windows, config["window"]["name"])(T, **config["window"].get("kwargs", {}))))
    if "filter" in config:
        sub = config["filter"]
        order = sub.get("order", 1)
        sections = []
        if "f_upper" in sub:
            sections.append(tp.bessel_sos(sub["f_upper"], fs, order, "low"))
        if "f_lower" in sub:
            sections.append(tp.bessel_sos(sub["f_lower"], fs, order, "high"))
        steps.append(("filter", np.concatenate(sections, axis=0) if sections else None))
    if "remove_modes" in config and config["remove_modes"]["modes_to_remove"] > 0:
        U, n = modes
        steps.append(("remove_modes", (np.asarray(U, float), np.asarray(n, float))))
    return steps


def _step(name, p, x, transpose):
    if name == "remove_slope":
        return slope_transpose(x) if transpose else slope(x)
    if name == "remove_spline":  # Q = I - B^T (B B^T)^-1 B on the time axis
        B, proj = p
        return x - (x @ B.T) @ proj if transpose else x - (x @ proj.T) @ B
    if name == "window":
        return x * p
    if name == "filter":  # H S;  H^T = J H J
        if transpose:
            u = x if p is None else scipy.signal.sosfilt(p, x[:, ::-1], axis=-1)[:, ::-1]
            return slope_transpose(u)
        s = slope(x)
        return s if p is None else scipy.signal.sosfilt(p, s, axis=-1)
    if name == "remove_modes":  # R = I - diag(n) U U^T diag(1/n)
        U, n = p
        if transpose:
            return x - (U @ (U.T @ (x * n[:, None]))) / n[:, None]
        return x - (U @ (U.T @ (x / n[:, None]))) * n[:, None]
    raise ValueError(name)


def apply(steps, x):
    x = np.asarray(x, np.float64)
    for name, p in steps:
        x = _step(name, p, x, False)
    return x


def apply_transpose(steps, x):
    x = np.asarray(x, np.float64)
    for name, p in reversed(steps):
        x = _step(name, p, x, True)
    return x
