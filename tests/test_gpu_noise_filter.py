"""mrx_tod_noise_filter against a float64 convolution, its symmetry, isolation and refusals, and the correlated-noise GLS
map of MaximumLikelihoodMapper(noise_model=...) against the white-noise map, a dense float64 solve and the destriper
(maria_amd/noise_filter.py).
The filter at the seams of its pair loop (carry registers, route edge, row lengths on block edges): tests/test_gpu_noise_seams.py."""

import ctypes as C

import numpy as np
import pytest
import scipy.signal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# per row: max |got - ref| over max (|k| * |s x|) s (the float32 transforms' error scales with the row's magnitudes)
ROW_TOL = 2e-6


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


def _run(ctx, x, ld, T, k, sw, ld_w, in_place):
    """the filter of the first T samples of x's rows (x [D, ld] host float32), sqrt_w sw ([rows, ld_w]) or None"""
    import torch

    from maria_amd._lib import ptr

    D = x.shape[0]
    d_x = _t(x, np.float32)
    d_y = d_x if in_place else torch.full((D, ld), 7.0, dtype=torch.float32, device=DEV)
    d_k = _t(k, np.float64)
    d_s = None if sw is None else _t(sw, np.float32)
    ctx.call("mrx_tod_noise_filter", ptr(d_x), ld, ptr(d_y), ld, D, T, ptr(d_k), k.shape[1] - 1, ptr(d_s), ld_w)
    torch.cuda.synchronize()
    y = d_y.cpu().numpy()
    if not in_place:
        assert np.all(y[:, T:] == 7.0)  # past T nothing is written
    return y[:, :T]


CASES = [  # D, T, K, ld pad, sqrt_w ("none", "shared", "rows"), in place
    (1, 100, 0, 0, "none", False),
    (3, 5000, 1, 3, "rows", True),
    (5, 3000, 16, 0, "shared", False),      # below one block (L = 4064)
    (4, 20011, 255, 5, "shared", True),     # not a multiple of the block
    (7, 300, 512, 0, "rows", False),        # T < 2 K
    (2, 1000, 1024, 1, "none", True),       # T < K
    (3, 77777, 1024, 0, "rows", False),
    (2, 240000, 2048, 0, "shared", True),
    (3, 5000, 2048, 2, "none", False),
    (65537, 61, 16, 3, "shared", True),     # D > 65535
]


@pytest.mark.parametrize("D,T,K,pad,sw_mode,in_place", CASES)
def test_filter_matches_a_float64_convolution(gpu_ctx, D, T, K, pad, sw_mode, in_place):
    """Worst row error measured on an MI355X over these cases: 4.1e-7 of max(|k| * |s x|) (K 255, T 20011); the bound is
    ROW_TOL = 2e-6."""
    rng = np.random.default_rng(K + D)
    ld = T + pad
    x = np.zeros((D, ld), np.float32)
    x[:, :T] = rng.normal(size=(D, T)) * rng.uniform(0.1, 10.0, (D, 1))
    x[0, :T] += 50.0  # an offset
    k = _lags(D, K, rng) if D < 1000 else np.tile(_lags(4, K, rng), (D // 4 + 1, 1))[:D]
    sw, ld_w, s = None, 0, np.ones((1, T))
    if sw_mode != "none":
        rows = 1 if sw_mode == "shared" else D
        sw = np.zeros((rows, ld), np.float32)
        sw[:, :T] = rng.uniform(0.0, 1.5, (rows, T))
        ld_w = 0 if sw_mode == "shared" else ld
        s = sw[:, :T].astype(np.float64)
    got = _run(gpu_ctx, x, ld, T, k, sw, ld_w, in_place)
    ref, mag = _reference(x[:, :T], k, s)
    err = np.abs(got - ref).max(axis=1) / np.maximum(mag, 1e-300)
    print(f"D {D} T {T} K {K}: worst row error {err.max():.2e} of max(|k| * |s x|)")
    assert err.max() <= ROW_TOL, (err.max(), int(err.argmax()))


def test_filter_is_symmetric(gpu_ctx):
    """<u, N^-1 v> = <N^-1 u, v> to float32 rounding (with a per-sample factor and a 1/f law)"""
    rng = np.random.default_rng(1)
    D, T, K = 6, 30000, 1500
    k = _lags(D, K, rng)
    k[::3] = _lags(D, K, rng)[1::3][: k[::3].shape[0]]
    sw = rng.uniform(0.2, 1.0, (1, T)).astype(np.float32)
    u, v = (rng.normal(size=(D, T)).astype(np.float32) for _ in range(2))
    nu, nv = (_run(gpu_ctx, a, T, T, k, sw, 0, False).astype(np.float64) for a in (u, v))
    lhs, rhs = np.sum(u * nv, axis=1), np.sum(nu * v, axis=1)
    scale = np.sum(np.abs(u) * np.abs(nv), axis=1)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (lhs - rhs) / scale


def test_a_nan_spoils_its_own_row_only(gpu_ctx):
    rng = np.random.default_rng(2)
    D, T, K = 5, 20000, 700
    x = rng.normal(size=(D, T)).astype(np.float32)
    k = _lags(D, K, rng)
    clean = _run(gpu_ctx, x, T, T, k, None, 0, False)
    x[2, 12345] = np.nan
    dirty = _run(gpu_ctx, x, T, T, k, None, 0, False)
    others = [0, 1, 3, 4]
    assert np.array_equal(clean[others], dirty[others])
    assert np.isnan(dirty[2]).any()


def test_refusals_leave_the_output_untouched(gpu_ctx):
    import torch

    from maria_amd._lib import ptr

    x = torch.zeros((4, 3000), dtype=torch.float32, device=DEV)
    y = torch.full((4, 3000), 7.0, dtype=torch.float32, device=DEV)
    k = torch.zeros((4, 2050), dtype=torch.float64, device=DEV)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    cases = {  # name: args
        "K 2049": (ptr(x), 3000, ptr(y), 3000, 4, 3000, ptr(k), 2049, None, 0),
        "K -1": (ptr(x), 3000, ptr(y), 3000, 4, 3000, ptr(k), -1, None, 0),
        "T 0": (ptr(x), 3000, ptr(y), 3000, 4, 0, ptr(k), 10, None, 0),
        "D 0": (ptr(x), 3000, ptr(y), 3000, 0, 3000, ptr(k), 10, None, 0),
        "ld < T": (ptr(x), 2999, ptr(y), 3000, 4, 3000, ptr(k), 10, None, 0),
        "null x": (None, 3000, ptr(y), 3000, 4, 3000, ptr(k), 10, None, 0),
        "null lags": (ptr(x), 3000, ptr(y), 3000, 4, 3000, None, 10, None, 0),
        "ld_w < T": (ptr(x), 3000, ptr(y), 3000, 4, 3000, ptr(k), 10, ptr(x), 100),
    }
    for name, args in cases.items():
        assert lib.mrx_tod_noise_filter(h, *args) == -1, name
    assert lib.mrx_tod_noise_filter(h, ptr(x), 3000, None, 3000, 4, 3000, ptr(k), 10, None, 0) == -1
    assert lib.mrx_tod_noise_filter(h, ptr(y), 3000, ptr(y), 2999, 4, 2999, ptr(k), 10, None, 0) == -1  # in place, ld differs
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


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


def test_white_law_gives_the_white_noise_map(gpu_ctx):
    """noise_model={"white": P_w, "knee": 0} is N^-1 = I / sigma^2 with sigma^2 = P_w fs / 2: the map of
    noise_weights = 1 / sigma^2 (nearest pointing: the exact per-pixel solve), within the CG tolerance.  Measured on an
    MI355X: 1.1e-7 of the map's maximum after one iteration; the bound is 1e-6."""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, az, el = _tods()
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="IQU", frame="az/el", tol=1e-9, max_iter=50)
    P_w = np.linspace(1e-6, 3e-6, tod.dets.n)
    sigma2 = P_w * 50.0 / 2
    white = MaximumLikelihoodMapper([tod], noise_weights=1.0 / sigma2, **kw)
    shape = (3, 1, white.n_eta, white.n_xi)
    rng = np.random.default_rng(5)
    tod.data = {"map": (_project(white, tod, _smooth_iqu(shape)).cpu().numpy()
                        + np.sqrt(sigma2)[:, None] * rng.normal(size=(tod.dets.n, tod.coords.t.size))).astype(np.float32)}
    m_white = white.run().data
    gls = MaximumLikelihoodMapper([tod], noise_model={"white": P_w, "knee": 0.0}, **kw)
    m_gls = gls.run().data
    assert gls.products["converged"]
    assert gls.products["noise_filter"][0]["K"] == 2048
    np.testing.assert_array_equal(np.isnan(m_white), np.isnan(m_gls))
    ok = np.isfinite(m_white)
    err = np.abs(m_gls[ok] - m_white[ok]).max() / np.abs(m_white[ok]).max()
    print(f"white limit: max |GLS - white| / max |white| = {err:.2e} after {gls.products['n_iter']} iterations")
    assert err <= 1e-6, err


@pytest.mark.parametrize("bilinear", [False, True])
def test_map_matches_a_dense_solve(gpu_ctx, bilinear):
    """D 48, T 6000, a 12 x 16 IQU map, a 1/f law (knee 1 Hz, alpha 1.5, K 2048): the map equals the float64 dense solve of
    P^T N^-1 P m = P^T N^-1 d on the solved pixels (P: the columns mrx_map_project gives for unit maps; N^-1: the Toeplitz
    blocks of the same host lags, applied by float64 convolution), each plane up to its hits-weighted mean.  Measured on
    an MI355X: 7.8e-8 (nearest, 37 iterations) and 7.3e-8 (bilinear, 28) of the dense map's maximum; the bound is 1e-6."""
    import scipy.sparse

    from maria_amd import noise_filter
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, az, el = _tods()
    D, T = tod.dets.n, tod.coords.t.size
    kw = dict(center=(az, el), width=16 * 0.05, height=12 * 0.05, resolution=0.05, stokes="IQU", frame="az/el", bilinear=bilinear,
              tol=1e-8, max_iter=400)
    law = {"white": 1e-4, "knee": 1.0, "alpha": 1.5}
    probe = MaximumLikelihoodMapper([tod], noise_model=law, **kw)
    shape = (3, 1, probe.n_eta, probe.n_xi)
    assert shape[2:] == (12, 16)
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
    d = (P @ _smooth_iqu(shape).ravel()).reshape(D, T) + 0.03 * np.cumsum(rng.normal(size=(D, T)), axis=1) / np.sqrt(T)
    d = d.astype(np.float32)
    tod.data = {"map": d}
    k = noise_filter.lags(law["white"], law["knee"], law["alpha"], 50.0, 2048).numpy()
    full = np.concatenate([k[:, :0:-1], k], axis=1)
    ninv = lambda v: scipy.signal.fftconvolve(v.reshape(D, T), full, axes=1)[:, 2048:2048 + T].ravel()  # noqa: E731
    PT = P.T.tocsr()
    A = np.stack([PT @ ninv(P[:, j].toarray().ravel()) for j in range(n)], axis=1)
    b = PT @ ninv(d.astype(np.float64).ravel())
    mapper = MaximumLikelihoodMapper([tod], noise_model=law, **kw)
    m = mapper.run().data
    assert mapper.products["converged"]
    solved = np.isfinite(m).ravel()
    assert solved.sum() > 0.8 * n
    ref = np.full(n, np.nan)
    ref[solved] = np.linalg.solve(A[np.ix_(solved, solved)], b[solved])
    ref, got = ref.reshape(shape), m.astype(np.float64)
    w = mapper.products["weight"][0, 0]
    err, scale = 0.0, 0.0
    for s in range(3):
        ok = np.isfinite(got[s, 0])
        r = got[s, 0][ok] - ref[s, 0][ok]
        r -= np.sum(w[ok] * r) / np.sum(w[ok])
        err = max(err, np.abs(r).max())
        scale = max(scale, np.abs(ref[s, 0][ok]).max())
    print(f"dense solve (bilinear {bilinear}): max |map - dense| / max |dense| = {err / scale:.2e}, "
          f"{mapper.products['n_iter']} iterations, |r|/|b| {mapper.products['residuals'][-1]:.1e}")
    assert err <= 1e-6 * scale, err / scale


def _two_band_sim(NEP, knee, duration=600.0, npos=150):
    """Simulation(noise=True) of a focal plane split into two groups of detectors (alternate positions), two bands at the
    same centre with their own NEP and knee, over the IQU blob map (test_gpu_noise_estimate's)."""
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
    noise_kwargs = {"correlated_noise_proportion": 0.0, "exact_spectrum": True}
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


def test_correlated_noise_gls_pays_on_a_mixed_focal_plane(gpu_ctx, capsys):
    """test_gpu_noise_estimate's two-group 1/f simulation (NEP 4e-16 and 8e-16, knees 2 and 20 Hz): the GLS map with the
    fitted law (noise_model="fit") against the white-noise GLS map with fitted weights and the destriper's best run there
    (fitted weights and prior, 0.32 s baselines).  Measured on an MI355X (noise seed 3): GLS 7.32e-4 K_RJ (51 iterations to
    |r|/|b| 9.3e-9), white-noise GLS 1.589e-3 (2.17x), destriper 9.148e-4 (1.25x, 45 iterations); the bounds are 1.5x
    and 1.05x."""
    from maria_amd.mappers import DestripingMapper, MaximumLikelihoodMapper

    tod, group, sky, centre, n, res = _two_band_sim((4e-16, 8e-16), (2.0, 20.0))
    kw = dict(center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="IQU", nu=[150e9], frame="ra/dec",
              units="K_RJ", tol=1e-8, max_iter=500)
    r, info = {}, {}
    runs = (("gls", MaximumLikelihoodMapper, dict(noise_model="fit")),
            ("white", MaximumLikelihoodMapper, dict(noise_weights="fit")),
            ("destriper", DestripingMapper, dict(noise_weights="fit", baseline_prior={"knee": "fit"}, baseline_length=0.32)))
    for name, cls, extra in runs:
        mapper = cls([tod], **kw, **extra)
        out = mapper.run()
        r[name] = _residual_rms(mapper, out, sky)
        info[name] = (mapper.products["n_iter"], mapper.products["residuals"][-1] if len(mapper.products["residuals"]) else 0.0,
                      mapper.products["converged"])
    with capsys.disabled():
        print("\nmixed focal plane, residual rms (K_RJ): " + ", ".join(f"{k} {v:.4e}" for k, v in r.items())
              + "; CG iterations, |r|/|b|, converged: " + ", ".join(f"{k} {v[0]} {v[1]:.1e} {v[2]}" for k, v in info.items()))
    assert info["gls"][2] and info["destriper"][2]
    assert r["white"] >= 1.5 * r["gls"], r
    assert r["gls"] <= 1.05 * r["destriper"], r
