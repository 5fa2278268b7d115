"""The mode-aware GLS map (maria_amd/noise_modes.py) on the device: mrx_tod_mode_project against float64
numpy, mrx_tod_noise_filter_modes against a float64 convolution of x - U b (and bit for bit the plain filter at m = 0),
the whole N^-1 against its dense Woodbury form, the map against the plain noise model, the input sky and a dense solve,
the fitted modes against the simulated couplings, and what the modes pay on a focal plane with shared noise.
The subtraction's tile edges and row-group loop and every row tail of the projection: tests/test_gpu_noise_seams.py."""

import ctypes as C

import numpy as np
import pytest
import scipy.signal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROW_TOL = 2e-6  # the plain filter's bound (tests/test_gpu_noise_filter.py)


def _t(a, dtype):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(DEV)


def _lags(D, K, rng):
    """a 1/f law's lags (positive definite) on most rows, random symmetric lags on every third"""
    from maria_amd import noise_filter

    k = noise_filter.lags(1.0, rng.uniform(0.5, 5.0, D), rng.uniform(0.5, 2.0, D), 50.0, K).numpy()
    k[::3] = rng.normal(size=(k[::3].shape))
    return k


def _reference(x, k, s):
    """s (k * (s x)) in float64 of the float32 rows, and the scale s (|k| * |s x|) of each row's rounding"""
    K = k.shape[1] - 1
    full = np.concatenate([k[:, :0:-1], k], axis=1)
    sx = x.astype(np.float64) * s
    y = scipy.signal.fftconvolve(sx, full, axes=1)[:, K:K + x.shape[1]] * s
    mag = scipy.signal.fftconvolve(np.abs(sx), np.abs(full), axes=1)[:, K:K + x.shape[1]] * np.abs(s)
    return y, mag.max(axis=1)


# ---- mrx_tod_mode_project ------------------------------------------------------------------------------------------

PROJECT_CASES = [  # D, T, m, ld pad
    (1, 1, 1, 0),
    (1, 1000, 16, 2),
    (7, 1, 5, 3),
    (7, 1000, 1, 0),
    (7, 1000, 5, 3),
    (7, 1000, 16, 1),
    (65537, 1000, 16, 1),
    (65537, 1, 5, 0),
    (3, 240000, 5, 2),
    (5, 240000, 16, 0),
    (2, 240000, 1, 7),
]


@pytest.mark.parametrize("D,T,m,pad", PROJECT_CASES)
def test_mode_project_matches_float64(gpu_ctx, D, T, m, pad):
    """a = U^T x against float64 numpy, the error bounded by 1e-13 of sum_d |U| |x| per sample"""
    import torch

    from maria_amd._lib import ptr

    rng = np.random.default_rng(D + T + m)
    ld = T + pad
    x = np.zeros((D, ld), np.float32)
    x[:, :T] = rng.normal(size=(D, T)) * rng.uniform(0.1, 10.0, (D, 1)) + 3.0
    U = rng.normal(size=(D, m))
    a = torch.full((m, T), 7.0, dtype=torch.float64, device=DEV)
    d_x, d_U = _t(x, np.float32), _t(U, np.float64)  # (held until the kernel has run)
    gpu_ctx.call("mrx_tod_mode_project", ptr(d_x), ld, D, T, ptr(d_U), m, ptr(a))
    torch.cuda.synchronize()
    xs = x[:, :T].astype(np.float64)
    ref = U.T @ xs
    mag = np.abs(U).T @ np.abs(xs)
    err = float((np.abs(a.cpu().numpy() - ref) / mag).max())
    print(f"mode project D {D} T {T} m {m}: worst error {err:.1e} of sum |U| |x|")
    assert err <= 1e-13, err


def test_mode_project_refusals_leave_the_output_untouched(gpu_ctx):
    import torch

    from maria_amd._lib import ptr

    x = torch.zeros((4, 300), dtype=torch.float32, device=DEV)
    U = torch.zeros((4, 17), dtype=torch.float64, device=DEV)
    a = torch.full((17, 300), 7.0, dtype=torch.float64, device=DEV)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    cases = {
        "null x": (None, 300, 4, 300, ptr(U), 2, ptr(a)),
        "null U": (ptr(x), 300, 4, 300, None, 2, ptr(a)),
        "null a": (ptr(x), 300, 4, 300, ptr(U), 2, None),
        "D 0": (ptr(x), 300, 0, 300, ptr(U), 2, ptr(a)),
        "T 0": (ptr(x), 300, 4, 0, ptr(U), 2, ptr(a)),
        "m 0": (ptr(x), 300, 4, 300, ptr(U), 0, ptr(a)),
        "m 17": (ptr(x), 300, 4, 300, ptr(U), 17, ptr(a)),
        "ld < T": (ptr(x), 299, 4, 300, ptr(U), 2, ptr(a)),
    }
    for name, args in cases.items():
        assert lib.mrx_tod_mode_project(h, *args) == -1, name
    torch.cuda.synchronize()
    assert bool((a == 7.0).all())


# ---- mrx_tod_noise_filter_modes ------------------------------------------------------------------------------------

def _run_modes(ctx, x, ld, T, k, sw, ld_w, in_place, U, b):
    """the filter of x - U b over the first T samples of x's rows (host float32 [D, ld]); U [D, m] or None (m = 0)"""
    import torch

    from maria_amd._lib import ptr

    D = x.shape[0]
    d_x = _t(x, np.float32)
    d_y = d_x if in_place else torch.full((D, ld), 7.0, dtype=torch.float32, device=DEV)
    d_k = _t(k, np.float64)
    d_s = None if sw is None else _t(sw, np.float32)
    m = 0 if U is None else U.shape[1]
    d_U = None if U is None else _t(U, np.float64)
    d_b = None if U is None else _t(b, np.float32)
    ctx.call("mrx_tod_noise_filter_modes", ptr(d_x), ld, ptr(d_y), ld, D, T, ptr(d_k), k.shape[1] - 1, ptr(d_s), ld_w, ptr(d_U), m, ptr(d_b))
    torch.cuda.synchronize()
    y = d_y.cpu().numpy()
    if not in_place:
        assert np.all(y[:, T:] == 7.0)
    return y[:, :T]


FILTER_CASES = [  # D, T, K, ld pad, sqrt_w, in place, m
    (1, 100, 0, 0, "none", False, 1),
    (3, 5000, 1, 3, "rows", True, 2),
    (5, 3000, 16, 0, "shared", False, 5),
    (4, 20011, 255, 5, "shared", True, 16),
    (7, 300, 512, 0, "rows", False, 3),
    (2, 1000, 1024, 1, "none", True, 2),
    (3, 77777, 1024, 0, "rows", False, 10),
    (2, 240000, 2048, 0, "shared", True, 5),
    (3, 5000, 2048, 2, "none", False, 16),
    (65537, 61, 16, 3, "shared", True, 4),
]


@pytest.mark.parametrize("D,T,K,pad,sw_mode,in_place,m", FILTER_CASES)
def test_filter_with_modes_matches_a_float64_convolution(gpu_ctx, D, T, K, pad, sw_mode, in_place, m):
    """s (k * (s (x - U b))) against the float64 reference of x - U b; the error per row over max(|k| * (|s| (|x| + |U||b|)))"""
    rng = np.random.default_rng(K + D + m)
    ld = T + pad
    x = np.zeros((D, ld), np.float32)
    x[:, :T] = rng.normal(size=(D, T)) * rng.uniform(0.1, 10.0, (D, 1))
    x[0, :T] += 50.0
    U = rng.normal(size=(D, m))
    b = (rng.normal(size=(m, T)) * 3.0).astype(np.float32)
    k = _lags(D, K, rng) if D < 1000 else np.tile(_lags(4, K, rng), (D // 4 + 1, 1))[:D]
    sw, ld_w, s = None, 0, np.ones((1, T))
    if sw_mode != "none":
        rows = 1 if sw_mode == "shared" else D
        sw = np.zeros((rows, ld), np.float32)
        sw[:, :T] = rng.uniform(0.0, 1.5, (rows, T))
        ld_w = 0 if sw_mode == "shared" else ld
        s = sw[:, :T].astype(np.float64)
    got = _run_modes(gpu_ctx, x, ld, T, k, sw, ld_w, in_place, U, b)
    b64 = b.astype(np.float64)
    ref, _ = _reference(x[:, :T].astype(np.float64) - U @ b64, k, s)
    _, mag = _reference(np.abs(x[:, :T]).astype(np.float64) + np.abs(U) @ np.abs(b64), k, s)
    err = np.abs(got - ref).max(axis=1) / np.maximum(mag, 1e-300)
    print(f"modes filter D {D} T {T} K {K} m {m}: worst row error {err.max():.2e}")
    assert err.max() <= ROW_TOL, (err.max(), int(err.argmax()))


@pytest.mark.parametrize("K,sw_mode", [(255, "shared"), (2048, "rows"), (1024, "none")])
def test_filter_with_no_modes_is_the_plain_filter_bit_for_bit(gpu_ctx, K, sw_mode):
    import torch

    from maria_amd._lib import ptr

    rng = np.random.default_rng(K)
    D, T = 5, 30011
    x = (rng.normal(size=(D, T)) * 4.0).astype(np.float32)
    k = _lags(D, K, rng)
    sw, ld_w = None, 0
    if sw_mode != "none":
        sw = rng.uniform(0.0, 1.5, (1 if sw_mode == "shared" else D, T)).astype(np.float32)
        ld_w = 0 if sw_mode == "shared" else T
    got = _run_modes(gpu_ctx, x, T, T, k, sw, ld_w, False, None, None)
    d_x, d_y = _t(x, np.float32), torch.empty((D, T), dtype=torch.float32, device=DEV)
    d_k, d_s = _t(k, np.float64), None if sw is None else _t(sw, np.float32)
    gpu_ctx.call("mrx_tod_noise_filter", ptr(d_x), T, ptr(d_y), T, D, T, ptr(d_k), K, ptr(d_s), ld_w)
    torch.cuda.synchronize()
    assert np.array_equal(got, d_y.cpu().numpy())
    # U = 0 with m > 0 filters x itself
    zero = _run_modes(gpu_ctx, x, T, T, k, sw, ld_w, True, np.zeros((D, 3)), rng.normal(size=(3, T)))
    assert np.array_equal(zero, got)


def test_filter_with_modes_refusals_leave_the_output_untouched(gpu_ctx):
    import torch

    from maria_amd._lib import ptr

    x = torch.zeros((4, 3000), dtype=torch.float32, device=DEV)
    y = torch.full((4, 3000), 7.0, dtype=torch.float32, device=DEV)
    k = torch.zeros((4, 2050), dtype=torch.float64, device=DEV)
    U = torch.zeros((4, 17), dtype=torch.float64, device=DEV)
    b = torch.zeros((17, 3000), dtype=torch.float32, device=DEV)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    base = (ptr(x), 3000, ptr(y), 3000, 4, 3000, ptr(k), 10, None, 0)
    cases = {
        "m 17": base + (ptr(U), 17, ptr(b)),
        "m -1": base + (ptr(U), -1, ptr(b)),
        "null U": base + (None, 2, ptr(b)),
        "null b": base + (ptr(U), 2, None),
        "K 2049": (ptr(x), 3000, ptr(y), 3000, 4, 3000, ptr(k), 2049, None, 0, ptr(U), 2, ptr(b)),
        "ld < T": (ptr(x), 2999, ptr(y), 3000, 4, 3000, ptr(k), 10, None, 0, ptr(U), 2, ptr(b)),
        "null lags": (ptr(x), 3000, ptr(y), 3000, 4, 3000, None, 10, None, 0, ptr(U), 2, ptr(b)),
    }
    for name, args in cases.items():
        assert lib.mrx_tod_noise_filter_modes(h, *args) == -1, name
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ---- the whole N^-1 ------------------------------------------------------------------------------------------------

def _toeplitz(k, T):
    t = np.arange(T)
    lagm = np.abs(t[:, None] - t[None, :])
    out = np.zeros((T, T))
    inside = lagm < k.size
    out[inside] = k[lagm[inside]]
    return out


def test_apply_matches_the_dense_woodbury_form(gpu_ctx):
    """D 6, T 256, m 2, K 40, s zero at both ends: N^-1 x against A' - A' U (B + U^T A' U)^-1 U^T A' in float64, its
    symmetry on random pairs and x^T N^-1 x > 0"""
    import torch

    from maria_amd import noise_filter, noise_modes

    rng = np.random.default_rng(11)
    D, T, m, K, fs = 6, 256, 2, 40, 50.0
    lag = noise_filter.lags(rng.uniform(0.5, 2.0, D), rng.uniform(0.5, 5.0, D), rng.uniform(0.8, 2.0, D), fs, K)
    beta = noise_filter.lags(rng.uniform(0.01, 0.05, m), rng.uniform(0.5, 5.0, m), 1.5, fs, K)
    U = rng.normal(size=(D, m))
    s = np.ones(T)
    s[:20] = s[-20:] = 0.0
    s[20:50] = np.linspace(0.0, 1.0, 30)
    A = np.zeros((D * T, D * T))
    for d in range(D):
        A[d * T:(d + 1) * T, d * T:(d + 1) * T] = s[:, None] * _toeplitz(lag[d].numpy(), T) * s[None, :]
    Ufull = np.kron(U, np.eye(T))  # [D T, m T]
    Bd = np.zeros((m * T, m * T))
    for j in range(m):
        Bd[j * T:(j + 1) * T, j * T:(j + 1) * T] = _toeplitz(beta[j].numpy(), T)
    AU = A @ Ufull
    Ninv = A - AU @ np.linalg.solve(Bd + Ufull.T @ AU, AU.T)
    d_lag, d_s = lag.to(DEV).contiguous(), _t(s, np.float32)
    model = noise_modes.ModeModel(_t(U, np.float64), beta.to(DEV).contiguous(), d_lag, d_s.double(), T, 1e-12)

    def apply(x):
        y = noise_modes.apply(gpu_ctx, _t(x, np.float32), d_lag, d_s, model)
        torch.cuda.synchronize()
        return y.cpu().numpy().astype(np.float64)

    xs = [rng.normal(size=(D, T)).astype(np.float32) for _ in range(4)]
    ys = [apply(x) for x in xs]
    for x, y in zip(xs, ys):
        ref = (Ninv @ x.astype(np.float64).ravel()).reshape(D, T)
        err = np.abs(y - ref).max() / np.abs(ref).max()
        print(f"N^-1 x: max error {err:.1e} of max |N^-1 x|; inner iterations {model.inner.iterations}")
        assert err <= 1e-5, err
        q = float(np.sum(x * y))
        assert q > 0, q
    for i in range(3):
        lhs, rhs = float(np.sum(xs[i] * ys[i + 1])), float(np.sum(ys[i] * xs[i + 1]))
        scale = float(np.sum(np.abs(xs[i]) * np.abs(ys[i + 1])))
        assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)
    assert np.linalg.eigvalsh(0.5 * (Ninv + Ninv.T)).min() >= -1e-10 * np.abs(Ninv).max()


# ---- the map -------------------------------------------------------------------------------------------------------

def _tods(D=48, T=6000, angles=(0.0, 45.0, 90.0, 135.0), seed=0, fov=0.4):
    """TODs (az/el frame) of a focal plane whose detectors take the given polarisation angles in turn (test_gpu_mlmap's)"""
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    t = 1.7e9 + np.arange(T) / 50.0
    az, el = synthetic.daisy_scan(t, radius_deg=0.3)
    pos = synthetic.hex_pack(D, np.radians(fov))
    bl = [Band(center=150e9, width=30e9, name="f150")]
    gamma = np.radians(np.asarray(angles))[np.arange(D) % len(angles)]
    dets = Detectors(pos, bl, np.zeros(D, int), gamma=gamma)
    coords = Coordinates(t, az, el, offsets=dets.offsets)
    return TOD({"map": np.zeros((dets.n, T), np.float32)}, dets, coords, units="K_RJ"), float(np.degrees(az.mean())), float(np.degrees(el.mean()))


def _project(mapper, tod, x):
    """P x with the mapper's inputs (mrx_map_project), [D, T] float32 on the device"""
    import torch

    from maria_amd._lib import Context, ptr

    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    signal, weight, az, el, tr, dx, dy, sw, chan = mapper._tod_inputs(tod, ctx, unit_i_response=mapper.units == "K_RJ")
    out = torch.empty_like(signal)
    D, T = signal.shape
    ctx.call("mrx_map_project", C.byref(mapper._sky()), ptr(_t(x, np.float64)), ptr(az), ptr(el), T, ptr(tr), ptr(dx), ptr(dy), ptr(sw),
             ptr(chan), D, 1.0, 0.0, ptr(out), T)
    torch.cuda.synchronize()
    return out


def _smooth_iqu(shape, seed=3):
    rng = np.random.default_rng(seed)
    S, Cn, ne, nx = shape
    E, X = np.meshgrid(np.linspace(-1, 1, ne), np.linspace(-1, 1, nx), indexing="ij")
    m = np.zeros(shape)
    for s in range(S):
        a, b, c = rng.normal(size=3)
        m[s, 0] = a * np.cos(2 * E + b) * np.sin(3 * X + c)
    return m


def _plane_err(got, ref, w):
    """max over the planes of |got - ref| on the solved pixels, each plane up to its w-weighted mean, and max |ref|"""
    err, scale = 0.0, 0.0
    for s in range(got.shape[0]):
        ok = np.isfinite(got[s, 0])
        r = got[s, 0][ok].astype(np.float64) - ref[s, 0][ok]
        r -= np.sum(w[ok] * r) / np.sum(w[ok])
        err = max(err, float(np.abs(r).max()))
        scale = max(scale, float(np.abs(ref[s, 0][ok]).max()))
    return err, scale


def _pattern(tod, m):
    """m smooth focal-plane patterns: a constant and gradients"""
    off = tod.dets.offsets / np.abs(tod.dets.offsets).max()
    cols = [np.ones(tod.dets.n), off[:, 0], off[:, 1], off[:, 0] * off[:, 1]]
    return np.stack(cols[:m], axis=1)


def test_zero_coupling_gives_the_plain_noise_model_map(gpu_ctx):
    """noise_model with modes U = 0 is N^-1 = A': the noise_model map within the CG tolerance"""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, az, el = _tods()
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="IQU", frame="az/el", tol=1e-9, max_iter=200)
    law = {"white": 1e-4, "knee": 1.0, "alpha": 1.5}
    plain = MaximumLikelihoodMapper([tod], noise_model=law, **kw)
    shape = (3, 1, plain.n_eta, plain.n_xi)
    rng = np.random.default_rng(5)
    tod.data = {"map": (_project(plain, tod, _smooth_iqu(shape)).cpu().numpy()
                        + 0.03 * np.cumsum(rng.normal(size=(tod.dets.n, tod.coords.t.size)), axis=1) / 50).astype(np.float32)}
    m_plain = plain.run().data
    modes = MaximumLikelihoodMapper([tod], noise_model=dict(law, modes=np.zeros((tod.dets.n, 2)), mode_law={"white": 1e-3, "knee": 0.5,
                                                                                                           "alpha": 1.0}), **kw)
    m_modes = modes.run().data
    assert modes.products["converged"]
    info = modes.products["noise_modes"][0]
    assert info["modes"].shape == (tod.dets.n, 2) and info["dropped"].size == 0
    np.testing.assert_array_equal(np.isnan(m_plain), np.isnan(m_modes))
    ok = np.isfinite(m_plain)
    err = np.abs(m_modes[ok] - m_plain[ok]).max() / np.abs(m_plain[ok]).max()
    print(f"U = 0: max |modes - plain| / max |plain| = {err:.2e} ({modes.products['n_iter']} vs {plain.products['n_iter']} iterations)")
    assert err <= 1e-6, err


def test_noiseless_sky_comes_back_where_remove_modes_does_not(gpu_ctx):
    """The GLS map with modes is unbiased: a noiseless sky TOD gives the input map back (each plane up to its weighted
    mean; the sky is zero on the pixels the map leaves out, whose signal N^-1 would otherwise spread over the others).
    The remove_modes pre-processing of a BinMapper on the same TOD does not."""
    from maria_amd.mappers import BinMapper, MaximumLikelihoodMapper

    tod, az, el = _tods()
    kw = dict(center=(az, el), width=0.9, resolution=0.05, frame="az/el")
    law = {"white": 1e-4, "knee": 0.1, "alpha": 1.0}
    U = 0.1 * _pattern(tod, 3)
    gls = MaximumLikelihoodMapper([tod], noise_model=dict(law, modes=U, mode_law={"white": 1e-3, "knee": 1.0, "alpha": 1.5}), stokes="IQU",
                                  tol=1e-10, max_iter=400, **kw)
    shape = (3, 1, gls.n_eta, gls.n_xi)
    sky = _smooth_iqu(shape)
    tod.data = {"map": _project(gls, tod, sky).cpu().numpy()}
    solved = np.isfinite(gls.run().data).all(axis=0, keepdims=True)
    sky = np.where(solved, sky, 0.0)
    tod.data = {"map": _project(gls, tod, sky).cpu().numpy()}
    out = gls.run().data
    assert gls.products["converged"]
    err, scale = _plane_err(out, sky, gls.products["weight"][0, 0])
    ctrl = MaximumLikelihoodMapper([tod], noise_model=law, stokes="IQU", tol=1e-10, max_iter=400, **kw)
    err_ctrl, _ = _plane_err(ctrl.run().data, sky, ctrl.products["weight"][0, 0])
    sky_i = sky.copy()
    sky_i[1:] = 0.0
    tod_i, _, _ = _tods()
    tod_i.data = {"map": _project(gls, tod_i, sky_i).cpu().numpy()}
    binned = BinMapper([tod_i], stokes="I", tod_preprocessing={"remove_modes": {"modes_to_remove": 3}}, **kw).run().data
    plain = BinMapper([tod_i], stokes="I", **kw).run().data
    w = np.isfinite(binned[0, 0]).astype(float)
    err_rm, scale_i = _plane_err(binned[:1], sky_i[:1], w)
    err_plain, _ = _plane_err(plain[:1], sky_i[:1], w)
    print(f"noiseless sky: GLS with modes {err / scale:.1e} of max |sky| ({gls.products['n_iter']} iterations, inner max "
          f"{gls.products['noise_modes'][0]['inner_iter_max']}); without modes {err_ctrl / scale:.1e} ({ctrl.products['n_iter']}); binned "
          f"{err_plain / scale_i:.1e}, binned after remove_modes {err_rm / scale_i:.1e}")
    assert err <= 1e-4 * scale, err / scale
    assert err_plain <= 1e-5 * scale_i
    assert err_rm >= 0.05 * scale_i, err_rm / scale_i


def test_map_with_modes_matches_a_dense_solve(gpu_ctx):
    """24 detectors x 2000 samples, m 2, an 8 x 10 IQU map (bilinear): the map equals the float64 solve of
    P^T N^-1 P m = P^T N^-1 d with N^-1 = A' - A' U (B + U^T A' U)^-1 U^T A' formed densely (the inner system factored)"""
    import scipy.linalg
    import scipy.sparse

    from maria_amd import noise_filter
    from maria_amd.mappers import MaximumLikelihoodMapper

    D, T, m, fs = 24, 2000, 2, 50.0
    tod, az, el = _tods(D=D, T=T)
    law = {"white": 1e-4, "knee": 1.0, "alpha": 1.5}
    mlaw = {"white": 1e-3, "knee": 2.0, "alpha": 1.2}
    U = 1e-2 * _pattern(tod, m)
    kw = dict(center=(az, el), width=10 * 0.06, height=8 * 0.06, resolution=0.06, stokes="IQU", frame="az/el", bilinear=True,
              tol=1e-9, max_iter=400, noise_filter_length=10.0)
    model = dict(law, modes=U, mode_law=mlaw)
    probe = MaximumLikelihoodMapper([tod], noise_model=model, **kw)
    shape = (3, 1, probe.n_eta, probe.n_xi)
    n = int(np.prod(shape))
    rows, cols, vals = [], [], []
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        pj = _project(probe, tod, e.reshape(shape)).cpu().numpy().ravel().astype(np.float64)
        nz = np.flatnonzero(pj)
        rows.append(nz)
        cols.append(np.full(nz.size, j))
        vals.append(pj[nz])
    P = scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(D * T, n))
    rng = np.random.default_rng(9)
    common = 0.05 * np.cumsum(rng.normal(size=(m, T)), axis=1) / np.sqrt(T)
    d = (P @ _smooth_iqu(shape).ravel()).reshape(D, T) + 0.02 * np.cumsum(rng.normal(size=(D, T)), axis=1) / np.sqrt(T) + U @ common
    d = d.astype(np.float32)
    tod.data = {"map": d}
    K = 500
    k = noise_filter.lags(law["white"], law["knee"], law["alpha"], fs, K).numpy()[0]
    beta = noise_filter.lags(mlaw["white"], mlaw["knee"], mlaw["alpha"], fs, K).numpy()[0]
    full = np.concatenate([k[:0:-1], k])
    aprime = lambda v: scipy.signal.fftconvolve(v.reshape(-1, T), full[None], axes=1)[:, K:K + T]  # noqa: E731
    Tk, Tb = _toeplitz(k, T), _toeplitz(beta, T)
    G = U.T @ U  # [m, m]: the lags are the same for every detector, G = (U^T U) k
    inner = np.kron(G, Tk) + np.kron(np.eye(m), Tb)
    fac = scipy.linalg.cho_factor(inner)

    def ninv(v):
        z = aprime(v)
        a = (U.T @ z).ravel()
        bsol = scipy.linalg.cho_solve(fac, a).reshape(m, T)
        return (z - aprime(U @ bsol)).ravel()

    PT = P.T.tocsr()
    A = np.stack([PT @ ninv(P[:, j].toarray().ravel()) for j in range(n)], axis=1)
    b = PT @ ninv(d.astype(np.float64).ravel())
    mapper = MaximumLikelihoodMapper([tod], noise_model=model, **kw)
    got = mapper.run().data
    assert mapper.products["converged"]
    assert mapper.products["noise_filter"][0]["K"] == K
    solved = np.isfinite(got).ravel()
    assert solved.sum() > 0.8 * n
    ref = np.full(n, np.nan)
    ref[solved] = np.linalg.solve(A[np.ix_(solved, solved)], b[solved])
    err, scale = _plane_err(got.astype(np.float64), ref.reshape(shape), mapper.products["weight"][0, 0])
    info = mapper.products["noise_modes"][0]
    print(f"dense solve with modes: max |map - dense| / max |dense| = {err / scale:.2e}, {mapper.products['n_iter']} iterations, "
          f"inner max {info['inner_iter_max']} total {info['inner_iter_total']}")
    assert err <= 1e-5 * scale, err / scale


# ---- the fit and what it pays --------------------------------------------------------------------------------------

def _one_band_sim(proportion=0.5, npos=150, duration=300.0):
    """Simulation(noise=True) of one band, no sky, in pW (the simulated coupling is then the spatial basis times one
    constant)"""
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation

    band = Band(center=150e9, width=40e9, name="f150", NEP=5e-16, knee=2.0)
    width = 1.0
    pos = synthetic.hex_pack(npos, np.radians(width / 2))
    dets = Detectors(pos, [band], np.zeros(npos, int), primary_size=1000.0, gamma=np.zeros(npos))
    plan = Plan.daisy(start_time=1.7e9, duration=duration, sample_rate=50.0, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
    sim = Simulation(Instrument(dets), plan, Site(altitude=5190.0), noise=True, noise_seed=3,
                     noise_kwargs={"correlated_noise_proportion": proportion, "exact_spectrum": True})
    (tod,) = sim.run(units="pW")
    return tod


def test_fitted_modes_span_the_simulated_couplings(gpu_ctx, capsys):
    """One band at the default correlated proportion 0.5, five simulated modes: the fitted U (m = 5) spans the spatial
    basis of maria_amd.noise (the cosines of the principal angles).  The basis's columns carry the square roots of the
    Matern kernel's eigenvalues, so its last two modes reach the detectors far weaker than the first three.  Measured on an
    MI355X (noise seed 3): cosines 0.9996, 0.9971, 0.9898, 0.799, 0.492; the bounds are 0.97 on the three leading ones and
    0.3 on all."""
    import torch

    from maria_amd import noise as mnoise
    from maria_amd import noise_modes
    from maria_amd._lib import Context
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod = _one_band_sim()
    offs = tod.dets.offsets
    basis = mnoise.spatial_basis(offs, k=5, n_side=16, scale=mnoise.diameter(offs) * 1.0)
    mapper = MaximumLikelihoodMapper([tod], center=(0.0, 0.0), width=1.0, resolution=0.1, units="pW", noise_model="fit", noise_modes=5)
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    signal = mapper._tod_inputs(tod, ctx)[0]
    fitted = noise_modes.fit(ctx, signal, 5, lambda rows: mapper._fit_noise(ctx, rows, tod))
    U = fitted["modes"].cpu().numpy()
    assert fitted["dropped"].size == 0 and U.shape == (tod.dets.n, 5)
    q1, _ = np.linalg.qr(U)
    q2, _ = np.linalg.qr(basis)
    cos = np.linalg.svd(q1.T @ q2, compute_uv=False)
    with capsys.disabled():
        print(f"\nfitted modes: principal-angle cosines against the simulated basis {np.array2string(cos, precision=4)}; mode laws "
              + ", ".join(f"{k} {np.array2string(v.cpu().numpy(), precision=3)}" for k, v in fitted["mode_law"].items()))
    assert cos[:3].min() >= 0.97, cos
    assert cos.min() >= 0.3, cos


def _two_band_sim(NEP, knee, proportion, duration=600.0, npos=150):
    """Simulation(noise=True) of a focal plane split into two groups of detectors (alternate positions), two bands at the
    same centre with their own NEP and knee, over the IQU blob map (test_gpu_noise_filter's, with the correlated
    proportion a parameter)."""
    from maria_amd import map as mmap
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation, sky_transform_stack
    from oracle import mapsample

    bands = [Band(center=150e9, width=40e9, name=f"f150{c}", NEP=nep, knee=k) for c, nep, k in zip("ab", NEP, knee)]
    width = 1.0
    pos = synthetic.hex_pack(npos, np.radians(width / 2))
    group = np.arange(npos) % 2
    gamma = np.radians([0.0, 45.0, 90.0, 135.0])[(np.arange(npos) // 2) % 4]
    dets = Detectors(pos, bands, group, primary_size=1000.0, gamma=gamma)
    plan = Plan.daisy(start_time=1.7e9, duration=duration, sample_rate=50.0, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
    site = Site(altitude=5190.0)
    noise_kwargs = {"correlated_noise_proportion": proportion, "exact_spectrum": True}
    transform = sky_transform_stack(plan.time, site.latitude, site.longitude)
    phi, theta = mapsample.frame_angles(plan.phi.astype(np.float32)[None], plan.theta.astype(np.float32)[None], transform)
    xyz = mapsample.phi_theta_to_xyz(phi[0], theta[0]).astype(float).mean(axis=0)
    xyz /= np.linalg.norm(xyz)
    centre = (float(np.arctan2(xyz[1], xyz[0]) % (2 * np.pi)), float(np.arcsin(xyz[2])))
    n = 32
    res = width / (n - 1)
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    blob = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0
    data = np.stack([s * blob[None] for s in (1.0, 0.2, -0.1)]).astype(np.float32)
    skymap = mmap.ProjectionMap(data, nu=[150e9], stokes="IQU", width=width, center=np.degrees(centre), frame="ra/dec")
    sim = Simulation(Instrument(dets), plan, site, map=skymap, noise=True, noise_seed=3, noise_kwargs=noise_kwargs)
    (tod,) = sim.run()
    return tod, group, skymap, centre, n, res


def _residual_rms(mapper, out, sky):
    """hits-weighted rms of (map - input) over the solved pixels and planes, each plane up to its weighted mean"""
    solved = np.isfinite(out.data[:, 0]).all(axis=0)
    w = mapper.products["weight"][0, 0][solved]
    tot = 0.0
    for s in range(3):
        r = out.data[s, 0][solved].astype(np.float64) - sky.data[s, 0][solved]
        r = r - np.sum(w * r) / np.sum(w)
        tot += np.sum(w * r * r) / np.sum(w)
    return float(np.sqrt(tot / 3))


def _payoff_runs(proportion, capsys):
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, group, sky, centre, n, res = _two_band_sim((4e-16, 8e-16), (2.0, 20.0), proportion)
    kw = dict(center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="IQU", nu=[150e9], frame="ra/dec",
              units="K_RJ", tol=1e-8, max_iter=500)
    r, info = {}, {}
    runs = (("modes", dict(noise_model="fit", noise_modes=10)), ("gls", dict(noise_model="fit")), ("white", dict(noise_weights="fit")))
    for name, extra in runs:
        mapper = MaximumLikelihoodMapper([tod], **kw, **extra)
        out = mapper.run()
        r[name] = _residual_rms(mapper, out, sky)
        inner = mapper.products.get("noise_modes", [{}])[0]
        info[name] = (mapper.products["n_iter"], mapper.products["residuals"][-1] if len(mapper.products["residuals"]) else 0.0,
                      mapper.products["converged"], inner.get("inner_iter_max", 0), inner.get("inner_iter_total", 0),
                      inner.get("dropped", np.zeros(0)).size)
    with capsys.disabled():
        print(f"\nproportion {proportion}: residual rms (K_RJ) " + ", ".join(f"{k} {v:.4e}" for k, v in r.items())
              + "; CG iterations, |r|/|b|, converged, inner max / total, dropped: "
              + ", ".join(f"{k} {v[0]} {v[1]:.1e} {v[2]} {v[3]}/{v[4]} {v[5]}" for k, v in info.items()))
    assert info["modes"][2] and info["gls"][2]
    return r


def test_modes_pay_where_the_noise_is_shared(gpu_ctx, capsys):
    """The two-group 1/f simulation at the default correlated proportion 0.5 (two bands: 2 x 5 shared modes):
    noise_model="fit", noise_modes=10 against noise_model="fit" alone and the white-noise GLS map.  Measured on an
    MI355X (noise seed 3): with modes 7.08e-4 K_RJ (82 CG iterations; inner solves of at most 14 iterations), without
    8.93e-4 (1.26x, 52 iterations), white-noise GLS 2.03e-3 (2.86x); the bounds are 1.15x and 2x."""
    r = _payoff_runs(0.5, capsys)
    assert r["gls"] >= 1.15 * r["modes"], r
    assert r["white"] >= 2.0 * r["modes"], r


def test_modes_cost_little_where_nothing_is_shared(gpu_ctx, capsys):
    """proportion 0.0 (tests/test_gpu_noise_filter.py's case): ten fitted modes cost at most 5 %.  Measured on an MI355X:
    7.310e-4 K_RJ with modes (58 CG iterations), 7.320e-4 without (51)."""
    r = _payoff_runs(0.0, capsys)
    assert r["modes"] <= 1.05 * r["gls"], r
