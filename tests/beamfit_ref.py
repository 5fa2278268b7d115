"""The beam fit restated in float64 numpy (maria_amd/beamfit.py): the composed pointing of steps 1-3, the
Gaussian beam model, its Jacobian as include/mrx.h writes it, the Gauss-Newton sums as one ``np.sum`` per row, and a
Levenberg-Marquardt on them.  No test file: the kernel tests and the host tests import it."""

import numpy as np

HALF_PI = np.pi / 2


def det_vector(dx, dy):
    """c [D, 3] = (-dy s, cos r, -dx s), s = sin r / r (transforms.py:14-23)."""
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    r = np.hypot(dx, dy)
    s = np.sinc(r / np.pi)
    return np.stack([-dy * s, np.cos(r), -dx * s], axis=-1)


def det_vector_jac(dx, dy):
    """(dc/ddx, dc/ddy), [D, 3] each, with h = (cos r - s) / r^2 (its series below r^2 = 0.09)."""
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    r2 = dx * dx + dy * dy
    r = np.sqrt(r2)
    s = np.sinc(r / np.pi)
    series = -1.0 / 3.0 + r2 * (1.0 / 30.0 + r2 * (-1.0 / 840.0 + r2 * (1.0 / 45360.0 + r2 * (-1.0 / 3991680.0))))
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(r2 < 0.09, series, (np.cos(r) - s) / np.where(r2 > 0, r2, 1.0))
    cx = np.stack([-dx * dy * h, -dx * s, -s - dx * dx * h], axis=-1)
    cy = np.stack([-s - dy * dy * h, -dy * s, -dx * dy * h], axis=-1)
    return cx, cy


def rotations(az, el, transform, center):
    """G [T, 3, 2]: dz = c @ G[t], the rotation of steps 1-3 composed per sample in float64 (mrx_map_pointing.h: sample_const).
    ``transform`` [T, 3, 3] or None; ``center`` (phi, theta) in radians."""
    az, el = np.asarray(az, np.float64), np.asarray(el, np.float64)
    a = el - HALF_PI
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(az), np.sin(az)
    zero = np.zeros_like(ca)
    R = np.stack([np.stack([ca * cb, ca * sb, sa], -1), np.stack([-sa * cb, -sa * sb, ca], -1), np.stack([-sb, cb, zero], -1)], axis=1)  # [T, 3, 3]
    M = np.broadcast_to(np.eye(3), (az.size, 3, 3)) if transform is None else np.asarray(transform, np.float64).reshape(-1, 3, 3)
    cphi, cth = float(center[0]), float(center[1])
    P = np.stack([-M[:, :, 0] * np.sin(cphi) + M[:, :, 1] * np.cos(cphi),
                  (M[:, :, 0] * np.cos(cphi) + M[:, :, 1] * np.sin(cphi)) * np.sin(cth) - M[:, :, 2] * np.cos(cth)], axis=-1)  # [T, 3, 2]
    return R @ P


def offsets(G, dx, dy, jac=False):
    """(ox, oy) [D, T] of detectors at (dx, dy) from the frame's centre; with ``jac`` also d(ox, oy)/d(dx, dy) as
    (oxx, oyx, oxy, oyy) = (dox/ddx, doy/ddx, dox/ddy, doy/ddy) with the asin(r)/r factor held constant."""
    dz = np.einsum("dk,tkj->dtj", det_vector(dx, dy), G)
    r = np.hypot(dz[..., 0], dz[..., 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(r > 0, np.arcsin(np.minimum(r, 1.0)) / np.where(r > 0, r, 1.0), 1.0)
    ox, oy = -dz[..., 0] * f, -dz[..., 1] * f
    if not jac:
        return ox, oy
    cx, cy = det_vector_jac(dx, dy)
    jx = -f[..., None] * np.einsum("dk,tkj->dtj", cx, G)
    jy = -f[..., None] * np.einsum("dk,tkj->dtj", cy, G)
    return ox, oy, (jx[..., 0], jx[..., 1], jy[..., 0], jy[..., 1])


def model(params, u, v):
    """(m, g, q) [D, T] at ``params`` [D, K], K = 5 (A, dx, dy, w, c) or 7 (A, dx, dy, a, b, cc, c)."""
    p = np.asarray(params, np.float64)
    K = p.shape[1]
    A, c = p[:, 0, None], p[:, K - 1, None]
    if K == 5:
        q = p[:, 3, None] * (u * u + v * v)
    else:
        q = p[:, 3, None] * (u * u) + 2.0 * p[:, 4, None] * (u * v) + p[:, 5, None] * (v * v)
    g = np.exp(-q / 2.0)
    return A * g + c, g, q


def jacobian(params, u, v, oj):
    """J [D, T, K] = dm/dparam by the formulas of include/mrx.h; ``oj`` the four derivatives of ``offsets``."""
    p = np.asarray(params, np.float64)
    K = p.shape[1]
    _, g, _ = model(p, u, v)
    Ag = p[:, 0, None] * g
    oxx, oyx, oxy, oyy = oj
    if K == 5:
        w = p[:, 3, None]
        mu, mv = -Ag * (w * u), -Ag * (w * v)
        shape = [-Ag * (u * u + v * v) / 2.0]
    else:
        a, b, cc = p[:, 3, None], p[:, 4, None], p[:, 5, None]
        mu, mv = -Ag * (a * u + b * v), -Ag * (b * u + cc * v)
        shape = [-Ag * (u * u) / 2.0, -Ag * (u * v), -Ag * (v * v) / 2.0]
    return np.stack([g, mu * oxx + mv * oyx, mu * oxy + mv * oyy, *shape, np.ones_like(g)], axis=-1)


def trial_offsets(params):
    """The trial (dx, dy) of every row as the device takes them: rounded to float32."""
    p = np.asarray(params, np.float64)
    return p[:, 1].astype(np.float32).astype(np.float64), p[:, 2].astype(np.float32).astype(np.float64)


def sums(x, G, params, flags=None, model_tod=None, src=None, shift=(0.0, 0.0), with_abs=False):
    """``(hits [D] int64, chi2 [D], JtJ [D, K, K], Jtr [D, K])`` over the samples whose flag is 0: an ``np.sum`` per row.
    ``shift`` moves every offset by (sx, sy) (the envelope of the kernel tests); ``with_abs`` appends the sums of the
    absolute terms (chi2, JtJ, Jtr) that bound the float64 rounding of a summation."""
    x = np.asarray(x, np.float64)
    D, T = x.shape
    keep = np.ones((D, T), bool) if flags is None else np.asarray(flags) == 0
    term = x if model_tod is None else x - np.asarray(model_tod, np.float64)
    dx, dy = trial_offsets(params)
    ox, oy, oj = offsets(G, dx, dy, jac=True)
    sx, sy = (0.0, 0.0) if src is None else (np.asarray(src, np.float64)[None, :, 0], np.asarray(src, np.float64)[None, :, 1])
    u, v = ox + shift[0] - sx, oy + shift[1] - sy
    with np.errstate(invalid="ignore", over="ignore"):  # (a trial step of the fit may leave the model's domain: its chi2 is then inf or NaN)
        m, _, _ = model(params, u, v)
        J = jacobian(params, u, v, oj)
        r = np.where(keep, term - m, 0.0)  # a flagged sample's value is selected away
        J = np.where(keep[..., None], J, 0.0)
        hits = keep.sum(axis=1).astype(np.int64)
        chi2 = np.sum(r * r, axis=1)
        JtJ = np.einsum("dti,dtj->dij", J, J)
        Jtr = np.einsum("dti,dt->di", J, r)
    if not with_abs:
        return hits, chi2, JtJ, Jtr
    return hits, chi2, JtJ, Jtr, (chi2, np.einsum("dti,dtj->dij", np.abs(J), np.abs(J)), np.einsum("dti,dt->di", np.abs(J), np.abs(r)))


def scales(p):
    """The natural size of a step of every parameter: (|A|, sigma, sigma, shape.., |A|), sigma from the shape terms."""
    K = p.shape[1]
    amp = np.abs(p[:, 0]) + 1e-300
    wmax = np.abs(p[:, 3]) if K == 5 else np.maximum(np.abs(p[:, 3]), np.abs(p[:, 5]))
    sigma = 1.0 / np.sqrt(wmax + 1e-300)
    return np.stack([amp, sigma, sigma] + [wmax + 1e-300] * (K - 4) + [amp], axis=1)


def positive_shape(p):
    K = p.shape[1]
    if K == 5:
        return p[:, 3] > 0
    return (p[:, 3] > 0) & (p[:, 5] > 0) & (p[:, 3] * p[:, 5] - p[:, 4] ** 2 > 0)


def lm_fit(normal, init, n_iter=20, tol=1e-8, min_hits=16, lam0=1e-3):
    """The Levenberg-Marquardt rule of ``beamfit.fit`` in numpy: ``normal(params) -> (hits, chi2, JtJ, Jtr)``.  Damping per
    detector, (JtJ + lam diag JtJ) step = Jtr; a step is accepted only where the detector's own chi2 fell (lam / 10;
    otherwise lam * 10); one ``normal`` call an iteration; a detector stops when an accepted step is below ``tol`` of
    ``scales`` and its chi2 fell by less than ``tol`` of itself.  Returns a dict of params, chi2, hits, cov, ok, converged."""
    p = np.array(init, np.float64)
    D, K = p.shape
    hits, chi2, JtJ, Jtr = normal(p)
    ok = (hits >= max(min_hits, K + 1)) & np.isfinite(chi2)
    lam = np.full(D, lam0)
    done = np.zeros(D, bool)
    eye = np.eye(K)
    for _ in range(n_iter):
        active = ok & ~done
        if not active.any():
            break
        step = np.zeros((D, K))
        for d in np.flatnonzero(active):
            Nd = JtJ[d] + lam[d] * np.diag(np.diag(JtJ[d]))
            try:
                step[d] = np.linalg.solve(Nd, Jtr[d])
            except np.linalg.LinAlgError:
                ok[d] = False
        active &= ok & np.isfinite(step).all(axis=1)
        trial = np.where(active[:, None], p + step, p)
        h2, c2, N2, r2 = normal(trial)
        better = active & (c2 < chi2) & positive_shape(trial)
        small = (np.abs(step) <= tol * scales(p)).all(axis=1) & (chi2 - c2 <= tol * chi2)
        done |= better & small
        done |= active & ~better & (np.abs(step) <= 1e-3 * tol * scales(p)).all(axis=1)  # nothing left to gain at this damping
        p = np.where(better[:, None], trial, p)
        chi2 = np.where(better, c2, chi2)
        JtJ = np.where(better[:, None, None], N2, JtJ)
        Jtr = np.where(better[:, None], r2, Jtr)
        lam = np.where(better, np.maximum(lam / 10.0, 1e-12), np.where(active, np.minimum(lam * 10.0, 1e12), lam))
    cov = np.full((D, K, K), np.nan)
    for d in np.flatnonzero(ok):
        try:
            cov[d] = np.linalg.inv(JtJ[d]) * chi2[d] / max(hits[d] - K, 1)
        except np.linalg.LinAlgError:
            ok[d] = False
    ok &= positive_shape(p) & np.isfinite(cov).all(axis=(1, 2))
    p = np.where(ok[:, None], p, np.nan)
    del eye
    return {"params": p, "chi2": np.where(ok, chi2, np.nan), "hits": hits, "cov": np.where(ok[:, None, None], cov, np.nan), "ok": ok,
            "converged": ok & done}


def fwhm_angle(a, b, cc):
    """(fwhm_major, fwhm_minor, angle) of the quadratic form q = a u^2 + 2 b u v + cc v^2: the eigenvalues l of
    [[a, b], [b, cc]] give sigma = 1 / sqrt(l); the major axis belongs to the smaller one; angle of the major axis from
    the u axis, in (-pi/2, pi/2]."""
    a, b, cc = (np.asarray(z, np.float64) for z in (a, b, cc))
    mean, diff = (a + cc) / 2.0, np.hypot((a - cc) / 2.0, b)
    l_small, l_big = mean - diff, mean + diff
    k = np.sqrt(8.0 * np.log(2.0))
    angle = 0.5 * np.arctan2(-2.0 * b, cc - a)
    angle = np.where(angle <= -HALF_PI, angle + np.pi, angle)
    return k / np.sqrt(l_small), k / np.sqrt(l_big), angle


# ---- the cases the host and the kernel tests share ---------------------------------------------------------------------

D_CASE, T_CASE = 19, 2 * 1024 + 37  # one full 16-row group plus three rows; two tiles of 1024 plus 37 samples
FWHM = np.radians(0.1)
SIGMA = FWHM / np.sqrt(8.0 * np.log(2.0))
RADIUS = 3.0 * FWHM
# The float32 spacing of the offsets' carriers.  The device forms (ox, oy) from float32 numbers of magnitude up to 1 (the
# detector's unit vector c, the sample's rotation G, cos and sin of the boresight elevation), each rounded at 2^-24 of 1,
# so the offsets live on the float32 grid at 1, whatever their own size: one spacing is 2^-23 rad (tests/test_gpu_map.py
# holds the same chain to 6e-7 rad, five of them).
SPACING = float(np.spacing(np.float32(1.0)))


def make_case(frame="az/el", drift=False, K=5, seed=0, D=D_CASE, T=T_CASE):
    """A daisy scan over a point source: boresight, frame, nominal and true offsets, true parameters, and the float32
    TOD with the model's own source in it (``beamfit.inject_source``: exact truth).  The last detector sits 5 degrees off
    the array and never crosses the source."""
    from maria_amd import beamfit, synthetic
    from maria_amd.sim import sky_transform_stack

    rng = np.random.default_rng(seed)
    t = 1.7e9 + np.arange(T) / 50.0
    az, el = synthetic.daisy_scan(t, radius_deg=0.35, speed_deg_s=0.6)
    az, el = az.astype(np.float32), el.astype(np.float32)
    if frame == "az/el":
        transform, center = None, (np.radians(45.0), np.radians(60.0))
    else:
        transform = sky_transform_stack(t, -23.0, -67.8)
        xyz = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1).astype(np.float64)
        mean = np.einsum("tk,tkj->tj", xyz, transform).mean(axis=0)
        mean /= np.linalg.norm(mean)
        center = (float(np.arctan2(mean[1], mean[0]) % (2 * np.pi)), float(np.arcsin(mean[2])))
    nominal = synthetic.hex_pack(D, np.radians(0.3))
    nominal[-1] = np.radians([5.0, 0.0])  # never crosses the source
    true_off = nominal + rng.normal(0.0, 0.15 * SIGMA, nominal.shape)
    A = rng.uniform(0.8, 1.2, D)
    c = rng.uniform(-0.05, 0.05, D)
    if K == 5:
        truth = np.stack([A, true_off[:, 0], true_off[:, 1], np.full(D, 1.0 / SIGMA**2) * rng.uniform(0.9, 1.1, D), c], axis=1)
    else:
        sM, sm, th = SIGMA * rng.uniform(1.05, 1.25, D), SIGMA * rng.uniform(0.8, 0.95, D), rng.uniform(-1.5, 1.5, D)
        lM, lm = 1.0 / sM**2, 1.0 / sm**2
        truth = np.stack([A, true_off[:, 0], true_off[:, 1], lM * np.cos(th) ** 2 + lm * np.sin(th) ** 2, np.cos(th) * np.sin(th) * (lM - lm),
                          lM * np.sin(th) ** 2 + lm * np.cos(th) ** 2, c], axis=1)
    src = None
    if drift:
        src = (np.linspace(-1.0, 1.0, T)[:, None] * np.radians([0.02, -0.015])[None, :]).astype(np.float32)
    x = beamfit.inject_source(np.zeros((D, T), np.float32), az, el, transform, center, truth, src=src)
    model_tod = (0.3 * np.sin(np.linspace(0.0, 5.0, T))[None, :] * np.linspace(0.5, 1.5, D)[:, None]).astype(np.float32)
    G = rotations(az, el, transform, center)
    ox, oy = offsets(G, nominal[:, 0].astype(np.float32), nominal[:, 1].astype(np.float32))
    if src is not None:
        ox, oy = ox - src[None, :, 0].astype(np.float64), oy - src[None, :, 1].astype(np.float64)
    return dict(t=t, az=az, el=el, transform=transform, center=center, nominal=nominal, truth=truth, x=x, model=model_tod, src=src, G=G,
                dist2=ox * ox + oy * oy, K=K, D=D, T=T)


def window_of(case, radius=RADIUS):
    """[D, T] uint8: 1 outside ``radius`` of the source at the nominal offsets (the fit's window is where it is 0)."""
    return (case["dist2"] > radius * radius).astype(np.uint8)


def start_of(case, rng=None):
    """A starting point [D, K] a fraction of the beam off the truth (the nominal offsets, the amplitude and the width 10 %
    off, c = 0): where ``fit_beams`` starts, and the trial point of the kernel tests."""
    tr = case["truth"]
    p = tr.copy()
    p[:, 0] *= 0.9
    p[:, 1:3] = case["nominal"]
    p[:, 3:-1] *= 1.1
    p[:, -1] = 0.0
    return p


def envelope(x, G, params, flags=None, model_tod=None, src=None, spacing=SPACING):
    """``(chi2, JtJ, Jtr)`` bounds on |kernel - reference| of the three sums: the change of the reference's own sum when
    every offset moves by +- one float32 spacing along ox, plus the same along oy (the larger of the two signs each),
    plus the float64 rounding of two summations of ``hits`` rounded terms, (hits + 8) 2^-52 sum|terms|."""
    hits, c0, N0, r0, ab = sums(x, G, params, flags, model_tod, src, with_abs=True)
    out = []
    for k, base in enumerate((c0, N0, r0)):
        e = 0.0
        for axis in (0, 1):
            d = []
            for sign in (1.0, -1.0):
                sh = (sign * spacing, 0.0) if axis == 0 else (0.0, sign * spacing)
                d.append(np.abs(sums(x, G, params, flags, model_tod, src, shift=sh)[1 + k] - base))
            e = e + np.maximum(d[0], d[1])
        h = (hits + 8.0).reshape((-1,) + (1,) * (base.ndim - 1))
        out.append(e + h * 2.0**-52 * ab[k])
    return tuple(out)


# ---- the cases of the edge tests (tests/test_gpu_beamfit_edges.py, tests/test_host_beamfit.py) -----------

def _frame_of(frame, t, az, el):
    """(transform, center) as ``make_case`` takes them: az/el about (45, 60) degrees, or ra/dec about the scan's mean."""
    from maria_amd.sim import sky_transform_stack

    if frame == "az/el":
        return None, (np.radians(45.0), np.radians(60.0))
    transform = sky_transform_stack(t, -23.0, -67.8)
    xyz = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1).astype(np.float64)
    mean = np.einsum("tk,tkj->tj", xyz, transform).mean(axis=0)
    mean /= np.linalg.norm(mean)
    return transform, (float(np.arctan2(mean[1], mean[0]) % (2 * np.pi)), float(np.arcsin(mean[2])))


def _truth_of(rng, offsets_true, K, minor=(0.8, 0.95)):
    """True parameters [D, K] with ``make_case``'s distributions at the true offsets."""
    D = offsets_true.shape[0]
    A = rng.uniform(0.8, 1.2, D)
    c = rng.uniform(-0.05, 0.05, D)
    if K == 5:
        return np.stack([A, offsets_true[:, 0], offsets_true[:, 1], np.full(D, 1.0 / SIGMA**2) * rng.uniform(0.9, 1.1, D), c], axis=1)
    sM, sm, th = SIGMA * rng.uniform(1.05, 1.25, D), SIGMA * rng.uniform(*minor, D), rng.uniform(-1.5, 1.5, D)
    lM, lm = 1.0 / sM**2, 1.0 / sm**2
    return np.stack([A, offsets_true[:, 0], offsets_true[:, 1], lM * np.cos(th) ** 2 + lm * np.sin(th) ** 2, np.cos(th) * np.sin(th) * (lM - lm),
                     lM * np.sin(th) ** 2 + lm * np.cos(th) ** 2, c], axis=1)


def _finish_case(t, az, el, transform, center, nominal, truth, src, K):
    from maria_amd import beamfit

    D, T = nominal.shape[0], t.size
    x = beamfit.inject_source(np.zeros((D, T), np.float32), az, el, transform, center, truth, src=src)
    model_tod = (0.3 * np.sin(np.linspace(0.0, 5.0, T))[None, :] * np.linspace(0.5, 1.5, D)[:, None]).astype(np.float32)
    G = rotations(az, el, transform, center)
    ox, oy = offsets(G, nominal[:, 0].astype(np.float32), nominal[:, 1].astype(np.float32))
    if src is not None:
        ox, oy = ox - src[None, :, 0].astype(np.float64), oy - src[None, :, 1].astype(np.float64)
    return dict(t=t, az=az, el=el, transform=transform, center=center, nominal=nominal, truth=truth, x=x, model=model_tod, src=src, G=G,
                dist2=ox * ox + oy * oy, K=K, D=D, T=T)


def make_offaxis_case(frame="az/el", K=5, common=(0.0, 0.0), center_shift=0.0, drift=False, seed=0, D=D_CASE, T=T_CASE):
    """``make_case`` with the hex-packed array moved by ``common`` (radians) on the focal plane and the frame's centre moved
    ``center_shift`` radians off the scan (in phi, divided by cos(theta)).  The source sits still where the array's mean
    lands in the frame (a constant float32 ``src`` track, plus ``make_case``'s linear drift with ``drift``), so the
    detectors still cross it.  The same keys as ``make_case``; no detector that never crosses the source."""
    from maria_amd import synthetic

    rng = np.random.default_rng(seed)
    t = 1.7e9 + np.arange(T) / 50.0
    az, el = synthetic.daisy_scan(t, radius_deg=0.35, speed_deg_s=0.6)
    az, el = az.astype(np.float32), el.astype(np.float32)
    transform, center = _frame_of(frame, t, az, el)
    center = (center[0] + center_shift / np.cos(center[1]), center[1])
    nominal = synthetic.hex_pack(D, np.radians(0.3)) + np.asarray(common, np.float64)[None, :]
    true_off = nominal + rng.normal(0.0, 0.15 * SIGMA, nominal.shape)
    truth = _truth_of(rng, true_off, K)
    G = rotations(az, el, transform, center)
    mean = nominal.mean(axis=0)
    mx, my = offsets(G, np.float32(mean[:1]), np.float32(mean[1:]))
    src = np.empty((T, 2), np.float64)
    src[:] = (mx.mean(), my.mean())
    if drift:
        src += np.linspace(-1.0, 1.0, T)[:, None] * np.radians([0.02, -0.015])[None, :]
    return _finish_case(t, az, el, transform, center, nominal, truth, src.astype(np.float32), K)


def make_hover_case(frame="az/el", K=5, D=17, T=1025, seed=0):
    """The boresight hovers over the source (the frame's centre: no ``src``): a Lissajous of 0.05 x 0.04 degrees about
    it, half a FWHM, with the array collapsed to within 0.2 FWHM of the boresight (the true offsets within 0.25), so that
    every sample of every row carries weight: exp(-q / 2) lies in [0.05, 1] at the truth and at ``start_of`` (asserted),
    and T = 1 or D = 1 still give sums of unit size.  The minor axis of K = 7 is 0.9 .. 1.0 sigma (``make_case``: 0.8 ..
    0.95), which keeps the far corner of the Lissajous above 0.05.  The same keys as ``make_case``."""
    from maria_amd import synthetic

    rng = np.random.default_rng(seed)
    t = 1.7e9 + np.arange(T) / 50.0
    ph = 2.0 * np.pi * np.arange(T) / 50.0
    az0, el0 = np.full(T, np.radians(45.0)), np.full(T, np.radians(60.0))
    if frame == "az/el":
        transform, center = None, (az0[0], el0[0])
    else:  # the source is fixed on the sky where (az0, el0) points at the first sample, and the boresight tracks it
        from maria_amd.sim import sky_transform_stack

        transform = sky_transform_stack(t, -23.0, -67.8)
        v = np.array([np.cos(az0[0]) * np.cos(el0[0]), np.sin(az0[0]) * np.cos(el0[0]), np.sin(el0[0])]) @ transform[0]
        center = (float(np.arctan2(v[1], v[0]) % (2 * np.pi)), float(np.arcsin(v[2])))
        b = np.einsum("j,tkj->tk", v, transform)
        az0, el0 = np.arctan2(b[:, 1], b[:, 0]), np.arcsin(b[:, 2])
    az = (az0 + np.radians(0.05) / np.cos(el0) * np.sin(0.37 * ph)).astype(np.float32)
    el = (el0 + np.radians(0.04) * np.sin(0.23 * ph + 0.5)).astype(np.float32)
    nominal = synthetic.hex_pack(D, 2 * 0.2 * FWHM)
    true_off = nominal + np.clip(rng.normal(0.0, 0.02 * FWHM, nominal.shape), -0.035 * FWHM, 0.035 * FWHM)
    truth = _truth_of(rng, true_off, K, minor=(0.9, 1.0))
    case = _finish_case(t, az, el, transform, center, nominal, truth, None, K)
    for p in (truth, start_of(case)):
        ox, oy = offsets(case["G"], *trial_offsets(p))
        g = model(p, ox, oy)[1]
        assert 0.05 <= g.min() and g.max() <= 1.0, (float(g.min()), float(g.max()))
    return case


def dz_radius(G, dx, dy):
    """|dz| [D, T], the r of the asin(r) / r factor: the kernel switches from its series to asinf at r^2 = 0.01."""
    dz = np.einsum("dk,tkj->dtj", det_vector(dx, dy), G)
    return np.hypot(dz[..., 0], dz[..., 1])


def mutant_JtJ(x, G, params, flags=None, src=None, f_one=False, h_zero=False):
    """JtJ [D, K, K] of ``sums`` with the Jacobian's factor asin(r) / r replaced by 1 (``f_one``) or the curvature term h
    of dc/d(dx, dy) by 0 (``h_zero``), the offsets themselves left alone: what a kernel wrong in that term alone would
    give.  With neither it is ``sums``' own JtJ."""
    x = np.asarray(x, np.float64)
    keep = np.ones(x.shape, bool) if flags is None else np.asarray(flags) == 0
    dx, dy = trial_offsets(params)
    ox, oy = offsets(G, dx, dy)
    r = dz_radius(G, dx, dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.ones_like(r) if f_one else np.where(r > 0, np.arcsin(np.minimum(r, 1.0)) / np.where(r > 0, r, 1.0), 1.0)
    cx, cy = det_vector_jac(dx, dy)
    if h_zero:
        s = np.sinc(np.hypot(dx, dy) / np.pi)
        zero = np.zeros_like(s)
        cx, cy = np.stack([zero, -dx * s, -s], axis=-1), np.stack([-s, -dy * s, zero], axis=-1)
    jx = -f[..., None] * np.einsum("dk,tkj->dtj", cx, G)
    jy = -f[..., None] * np.einsum("dk,tkj->dtj", cy, G)
    sx, sy = (0.0, 0.0) if src is None else (np.asarray(src, np.float64)[None, :, 0], np.asarray(src, np.float64)[None, :, 1])
    J = jacobian(params, ox - sx, oy - sy, (jx[..., 0], jx[..., 1], jy[..., 0], jy[..., 1]))
    J = np.where(keep[..., None], J, 0.0)
    return np.einsum("dti,dtj->dij", J, J)


# The off-axis cases of DESIGN 3.31 at D_CASE x T_CASE: the builder's arguments, then how the kernel test runs them (model,
# layout) and which term of the Jacobian each makes visible (the mutants of ``mutant_JtJ`` that must move JtJ).
# Case 3 sits at (0.06, 0.04) rad: at (0.03, 0.02) h = 0 moves JtJ by 3.0 .. 43 envelopes, under 8 in five of the 18 rows.
OFFAXIS = {
    1: dict(make=dict(frame="az/el", K=5, center_shift=0.122), with_model=False, layout="aligned", mutants=("f_one",)),
    2: dict(make=dict(frame="ra/dec", K=7, center_shift=0.1002), with_model=True, layout="odd", mutants=("f_one",)),
    3: dict(make=dict(frame="az/el", K=7, common=(0.06, 0.04), drift=True), with_model=False, layout="odd", mutants=("h_zero",)),
    4: dict(make=dict(frame="ra/dec", K=5, common=(0.2, 0.25)), with_model=True, layout="aligned", mutants=("h_zero",)),
    5: dict(make=dict(frame="az/el", K=5, common=(0.2, 0.224)), with_model=False, layout="odd", mutants=("h_zero",)),
    6: dict(make=dict(frame="ra/dec", K=7, common=(0.2, 0.25), center_shift=0.122, drift=True), with_model=True, layout="aligned",
            mutants=("f_one", "h_zero")),
}
_OFFAXIS_MADE = {}


def offaxis_case(number):
    """(case, flags, params) of an off-axis case, made once and never changed: the window at the nominal offsets with
    row 3 flagged end to end and every seventh sample of row 5 flagged with another bit; the trial point ``start_of``."""
    if number not in _OFFAXIS_MADE:
        case = make_offaxis_case(**OFFAXIS[number]["make"])
        flags = window_of(case)
        flags[3] = 1
        flags[5, ::7] = 4
        _OFFAXIS_MADE[number] = (case, flags, start_of(case))
    return _OFFAXIS_MADE[number]


def offaxis_geometry(number):
    """Asserts that the case's samples lie where DESIGN 3.31 says they do (which branch of the kernel each takes), and
    returns the figures as a string."""
    case, flags, params = offaxis_case(number)
    dx, dy = trial_offsets(params)
    r2 = dz_radius(case["G"], dx, dy) ** 2
    kept = r2[flags == 0]
    d2 = dx.astype(np.float32) ** 2 + dy.astype(np.float32) ** 2  # the float32 sum the row's DetConst branches on
    assert np.abs(d2.astype(np.float64) - 0.09).min() > 1e-5  # no row on the threshold itself, in float32 or float64
    if number in (1, 6):
        assert r2.min() > 0.0101  # every sample of every row past the switch to asinf
    if number == 2:
        assert (kept < 0.01).mean() >= 0.1 and (kept >= 0.01).mean() >= 0.1
    if number == 3:
        assert d2.max() < 0.09 and d2.min() > 4e-3 and r2.max() < 0.01  # both series, with a visible h
    if number in (4, 6):
        assert np.all(d2 >= np.float32(0.09))
    if number == 5:
        assert (d2 < np.float32(0.09)).sum() >= 3 and (d2 >= np.float32(0.09)).sum() >= 3
    return (f"case {number}: |dz|^2 of kept samples {kept.min():.4f} .. {kept.max():.4f} ({100 * (kept < 0.01).mean():.0f} % below 0.01); "
            f"dx^2 + dy^2 {d2.min():.4f} .. {d2.max():.4f} ({int((d2 < np.float32(0.09)).sum())} rows below 0.09)")


D_PROBE, T_PROBE = 33, 2 * 16384 + 1024 + 5  # three groups of rows, the last of one row; three chunks, the last of two tiles
# lane 0 and lane 63, q = 0 and 3, every wave's edge in a tile, both chunk seams, the last tile's byte-wise tail
PROBE_POSITIONS = (0, 1, 3, 4, 252, 255, 256, 259, 1020, 1023, 1024, 1027, 16380, 16383, 16384, 16387, 32767, 32768, T_PROBE - 5, T_PROBE - 4,
                   T_PROBE - 1)


def probe_flags(rotate):
    """(flags [D_PROBE, T_PROBE] of ones with a single 0 a live row, kept [D_PROBE] the position or -1): rows 0 .. 15, 31 and
    32 keep PROBE_POSITIONS[(row + rotate) mod 21]; rows 16 .. 30 keep nothing, so the second group of 16 runs on row 31
    alone."""
    flags = np.ones((D_PROBE, T_PROBE), np.uint8)
    kept = np.full(D_PROBE, -1)
    for j, d in enumerate(list(range(16)) + [31, 32]):
        kept[d] = PROBE_POSITIONS[(j + rotate) % len(PROBE_POSITIONS)]
        flags[d, kept[d]] = 0
    return flags, kept


def seeded_flags(D, T, seed):
    """[D, T] uint8: runs of random length covering about 30 % of every row plus isolated single flags (2 %), in the values
    1, 4 and 128; below T = 8 every sample is flagged with probability 0.3."""
    rng = np.random.default_rng(seed)
    values = np.array([1, 4, 128], np.uint8)
    f = np.zeros((D, T), np.uint8)
    for d in range(D):
        if T < 8:
            f[d] = np.where(rng.random(T) < 0.3, rng.choice(values, T), 0)
            continue
        while (f[d] != 0).mean() < 0.3:
            a = int(rng.integers(T))
            f[d, a:a + int(rng.integers(1, max(2, min(T // 4, 400))))] = rng.choice(values)
        single = rng.random(T) < 0.02
        f[d, single] = rng.choice(values, int(single.sum()))
    return f
