"""The destriper's baseline prior on the device: mrx_baseline_prior_apply against the dense Laplacian,
mrx_baseline_band_factor + mrx_baseline_band_solve against scipy.linalg.solveh_banded, the refused arguments, and
DestripingMapper(baseline_prior=...) against a dense solve of its normal equations, in its two limits and on the
1/f-dominated simulation.  The builders are the maximum-likelihood and destriper tests' own."""

import ctypes as C

import numpy as np
import pytest
import scipy.linalg
from test_gpu_destripe import _front_end_1f, _residual_rms
from test_gpu_mlmap import DEV, _fill_with_projection, _iqu_map, _t, _tods

from maria_amd import destripe_prior as dp

pytestmark = pytest.mark.gpu


def _apply(ctx, w, scale, hits, a):
    import torch

    from maria_amd._lib import ptr

    D, nb = a.shape
    y = torch.full((D, nb), float("nan"), dtype=torch.float64, device=DEV)
    d_hits = None if hits is None else _t(hits, np.float64)
    d_w, d_s, d_a = _t(w, np.float64), _t(scale, np.float64), _t(a, np.float64)  # (held until the kernel has run)
    ctx.call("mrx_baseline_prior_apply", D, nb, len(w), ptr(d_w), ptr(d_s), ptr(d_hits), ptr(d_a), ptr(y))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _factor_solve(ctx, w, scale, hits, r, Kp):
    import torch

    from maria_amd._lib import ptr

    D, nb = r.shape
    fac = torch.full((max(D * nb * (Kp + 1), 1),), float("nan"), dtype=torch.float64, device=DEV)
    ok = torch.full((D,), 7, dtype=torch.uint8, device=DEV)
    d_w, d_s, d_h, d_r = _t(w, np.float64), _t(scale, np.float64), _t(hits, np.float64), _t(r, np.float64)  # (held)
    ctx.call("mrx_baseline_band_factor", D, nb, Kp, ptr(d_w), ptr(d_s), ptr(d_h), ptr(fac), ptr(ok))
    z = torch.full((D, nb), float("nan"), dtype=torch.float64, device=DEV)
    ctx.call("mrx_baseline_band_solve", D, nb, Kp, ptr(fac), ptr(ok), ptr(d_r), ptr(z))
    torch.cuda.synchronize()
    return z.cpu().numpy(), ok.cpu().numpy()


@pytest.mark.parametrize("K", [1, 2, 5, 16, 33, 64])
@pytest.mark.parametrize("nb", [1, 3, 40, 257, 700])
def test_prior_apply_matches_the_dense_laplacian(gpu_ctx, K, nb):
    """y = hits a + s_d T a against the dense T for random signed weights and scales (one of them 0), nb < K, nb = 1,
    several tiles; without hits; and T 1 = 0 exactly."""
    rng = np.random.default_rng(K * 1000 + nb)
    D = 6
    w = rng.normal(size=K)
    scale = rng.uniform(0.0, 3.0, D)
    scale[2] = 0.0
    hits = rng.uniform(0.0, 20.0, (D, nb)) * (rng.uniform(size=(D, nb)) < 0.8)
    a = rng.normal(size=(D, nb))
    T = dp.laplacian(w, nb)
    ref = hits * a + scale[:, None] * (a @ T.T)
    got = _apply(gpu_ctx, w, scale, hits, a)
    assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
    got0 = _apply(gpu_ctx, w, scale, None, a)
    assert np.abs(got0 - scale[:, None] * (a @ T.T)).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
    const = np.repeat(rng.normal(size=(D, 1)), nb, axis=1)
    assert np.array_equal(_apply(gpu_ctx, w, scale, None, const), np.zeros((D, nb)))  # T 1 = 0 exactly


def _band_ref(w, s, h, r, Kp):
    """scipy.linalg.solveh_banded of diag(h) + s T_Kp (upper form)."""
    nb = len(h)
    A = np.diag(h) + s * dp.laplacian(w[:Kp], nb)
    kb = min(Kp, nb - 1)  # (the band cannot be wider than the matrix)
    ab = np.zeros((kb + 1, nb))
    for j in range(kb + 1):
        ab[kb - j, j:] = np.diagonal(A, j)
    return scipy.linalg.solveh_banded(ab, r)


@pytest.mark.parametrize("Kp", [0, 1, 4, 16])
@pytest.mark.parametrize("nb", [1, 3, 40, 300])
def test_band_factor_and_solve_match_solveh_banded(gpu_ctx, Kp, nb):
    """z = (diag(hits) + s T_Kp)^-1 r for the prior's own weights (alpha = 1, L = 16), baselines with no hits among
    them; a detector with no hits at all (and, at Kp = 0, any detector with a baseline without hits) has ok = 0, z = 0."""
    rng = np.random.default_rng(Kp * 100 + nb)
    D = 70  # two workgroups of the factor and the solve
    w = dp.prior_weights(50.0, 16, 1.0, 300)
    scale = rng.uniform(0.1, 3.0, D)
    hits = rng.uniform(1.0, 20.0, (D, nb)) * (rng.uniform(size=(D, nb)) < 0.7)
    hits[:, 0] = np.where(np.arange(D) % 3 == 0, 0.0, hits[:, 0])
    hits[5] = 0.0
    hits[66, nb // 2] = 4.0  # (a hit somewhere in the second workgroup's row)
    r = rng.normal(size=(D, nb))
    z, ok = _factor_solve(gpu_ctx, w, scale, hits, r, Kp)
    assert set(np.unique(ok)) <= {0, 1}
    for d in range(D):
        expect_ok = hits[d].any() and (Kp > 0 and nb > 1 or (hits[d] > 0).all())
        assert ok[d] == expect_ok, (d, ok[d], hits[d])
        if ok[d]:
            ref = _band_ref(w, scale[d], hits[d], r[d], Kp)
            assert np.abs(z[d] - ref).max() <= 1e-10 * np.abs(ref).max(), d
        else:
            assert np.all(z[d] == 0.0)


def test_refused_arguments_leave_the_context_usable(gpu_ctx):
    import torch

    from maria_amd._lib import MrxError, ptr

    D, nb = 4, 50
    w, scale = _t(np.ones(64), np.float64), _t(np.ones(D), np.float64)
    a, y = _t(np.ones((D, nb)), np.float64), torch.zeros((D, nb), dtype=torch.float64, device=DEV)
    fac, ok = torch.zeros(D * nb * 17, dtype=torch.float64, device=DEV), torch.zeros(D, dtype=torch.uint8, device=DEV)
    for K in (0, 65):
        with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
            gpu_ctx.call("mrx_baseline_prior_apply", D, nb, K, ptr(w), ptr(scale), None, ptr(a), ptr(y))
    with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
        gpu_ctx.call("mrx_baseline_prior_apply", D, 0, 4, ptr(w), ptr(scale), None, ptr(a), ptr(y))
    for Kp in (-1, 17):
        with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
            gpu_ctx.call("mrx_baseline_band_factor", D, nb, Kp, ptr(w), ptr(scale), ptr(a), ptr(fac), ptr(ok))
        with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
            gpu_ctx.call("mrx_baseline_band_solve", D, nb, Kp, ptr(fac), ptr(ok), ptr(a), ptr(y))
    with pytest.raises(MrxError, match="MRX_ERR_INVALID"):
        gpu_ctx.call("mrx_baseline_band_solve", D, 0, 4, ptr(fac), ptr(ok), ptr(a), ptr(y))
    for bad in (-1.0, float("nan")):
        neg = _t([1.0, 2.0, bad, 1.0], np.float64)
        with pytest.raises(MrxError, match="scale"):
            gpu_ctx.call("mrx_baseline_prior_apply", D, nb, 4, ptr(w), ptr(neg), None, ptr(a), ptr(y))
        with pytest.raises(MrxError, match="scale"):
            gpu_ctx.call("mrx_baseline_band_factor", D, nb, 4, ptr(w), ptr(neg), ptr(a), ptr(fac), ptr(ok))
    # the context still works
    gpu_ctx.call("mrx_baseline_prior_apply", D, nb, 4, ptr(w), ptr(scale), ptr(a), ptr(a), ptr(y))
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), np.ones((D, nb)))


# ---- DestripingMapper(baseline_prior=...) ----


def _kernel_pixels(mapper, tod):
    """The pixel of every sample as the mapper's kernels see it: mrx_map_project of an index map through the mapper's own
    pointing inputs (one channel)."""
    import torch

    from maria_amd._lib import Context, MrxSkyMap, ptr

    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    signal, _, az, el, tr, dx, dy, _, chan = mapper._tod_inputs(tod, ctx, unit_i_response=True)
    s = mapper._sky()
    sky1 = MrxSkyMap(None, 1, 1, s.n_eta, s.n_xi, s.eta0, s.deta, s.xi0, s.dxi, s.center_phi, s.center_theta, 0, 0)
    idx = _t(np.arange(s.n_eta * s.n_xi, dtype=np.float64).reshape(1, 1, s.n_eta, s.n_xi), np.float64)
    D, T = signal.shape
    ones = _t(np.ones((D, 1)), np.float64)
    out = torch.empty((D, T), dtype=torch.float32, device=DEV)
    ctx.call("mrx_map_project", C.byref(sky1), ptr(idx), ptr(az), ptr(el), T, ptr(tr), ptr(dx), ptr(dy), ptr(ones), ptr(chan), D, 1.0,
             0.0, ptr(out), out.stride(0))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _gauge(a, hits, sw, every_baseline=True):
    """The mapper's gauge: a made hits-orthogonal to g_k[d][b] = sw[d, k] (one channel)."""
    G = np.einsum("dk,dl,d->kl", sw, sw, hits.sum(axis=1))
    n = sw.T @ (hits * a).sum(axis=1)
    c = np.linalg.pinv(G, rcond=1e-12) @ n
    seen = hits.any(axis=1, keepdims=True) if every_baseline else hits > 0
    return a - np.where(seen, (sw @ c)[:, None], 0.0)


def _setup(D=16, T=1600, seed=6, amp=5.0):
    from maria_amd.mappers import DestripingMapper

    tod, caz, cel = _tods(D=D, T=T)
    kw = dict(center=(caz, cel), width=0.8, resolution=0.8 / 12, stokes="IQU", nu=150e9, frame="az/el", units="K_RJ")
    probe = DestripingMapper([tod], baseline_length=0.32, **kw)
    m_true = _iqu_map(probe)
    _fill_with_projection(probe, [tod], m_true)
    rng = np.random.default_rng(seed)
    drift = np.cumsum(rng.normal(size=(tod.dets.n, T)), axis=1) * amp / np.sqrt(T)  # a random walk: red offsets
    tod.data["map"] = (tod.data["map"] + drift + 0.05 * rng.normal(size=drift.shape)).astype(np.float32)
    return tod, kw


def test_prior_offsets_equal_a_dense_solve(gpu_ctx):
    """On a small problem (16 detectors x 1600 samples, 16-sample baselines, 100 a detector, per-detector weights and
    knees) the offsets equal a dense solve of (F^T W mu F - F^T W mu P M^+ P^T W F + S T) a = F^T W mu (d - P m0), after
    the same gauge fix, to 1e-8 of their largest value; the map equals m0 - M^-1 P^T W F a to 1e-8 of its largest value."""
    import scipy.sparse

    from maria_amd.map import mueller_row
    from maria_amd.mappers import DestripingMapper

    tod, kw = _setup()
    D, T = tod.data["map"].shape
    rng = np.random.default_rng(1)
    W = rng.uniform(0.5, 2.0, D).astype(np.float32).astype(np.float64)  # (the binning of P^T W d takes W in float32)
    knee = rng.uniform(0.3, 3.0, D)
    mapper = DestripingMapper([tod], baseline_length=0.32, noise_weights=W, tol=1e-12, max_iter=3000,
                              baseline_prior={"knee": knee, "alpha": 1.0, "band": 8}, **kw)
    out = mapper.run()
    pr = mapper.products
    assert pr["converged"], pr["residuals"][-5:]
    L = mapper.baseline_samples[0]
    nb = -(-T // L)
    prior = pr["prior"][0]
    w = prior["weights"]
    assert prior["K"] == len(w) and prior["Kp"] == 8 and np.array_equal(w, dp.prior_weights(mapper.sample_rates[0], L, 1.0, nb))
    # the dense system, from the kernels' own pixels
    pix = _kernel_pixels(mapper, tod)
    solved = np.isfinite(out.data[0, 0]).ravel()
    n_pix = solved.size
    cols = np.nonzero(solved)[0]
    where = np.full(n_pix, -1)
    where[cols] = np.arange(cols.size)
    sw = mueller_row(tod.dets.gamma)
    sw = sw[:, :3] / sw[:, :1]
    mu = solved[pix].astype(np.float64)  # [D, T]
    rows = np.arange(D * T)
    keep = mu.ravel() > 0
    P = scipy.sparse.hstack([scipy.sparse.csr_matrix((np.repeat(sw[:, k], T)[keep], (rows[keep], where[pix.ravel()[keep]])),
                                                     shape=(D * T, cols.size)) for k in range(3)]).tocsr()  # mu P
    F = scipy.sparse.csr_matrix((np.ones(D * T), (rows, (np.arange(D)[:, None] * nb + np.arange(T)[None, :] // L).ravel())),
                                shape=(D * T, D * nb))
    Wt = scipy.sparse.diags(np.repeat(W, T) * mu.ravel())
    Mm = (P.T @ Wt @ P).toarray()
    B = (P.T @ Wt @ F).toarray()
    d = tod.data["map"].astype(np.float64).ravel()
    m0 = np.linalg.solve(Mm, P.T @ (Wt @ d))
    s = W / knee
    ST = scipy.linalg.block_diag(*[s_d * dp.laplacian(w, nb) for s_d in s])
    A = (F.T @ Wt @ F).toarray() - B.T @ np.linalg.solve(Mm, B) + ST
    rhs = F.T @ (Wt @ (d - P @ m0))
    a_ref = np.linalg.lstsq(A, rhs, rcond=1e-13)[0].reshape(D, nb)
    hits = pr["hits"][0]
    np.testing.assert_allclose(hits, (F.T @ (Wt @ np.ones(D * T))).reshape(D, nb), rtol=1e-12)
    a_ref = _gauge(a_ref, hits, sw)
    got = pr["baselines"][0]
    assert np.abs(got - a_ref).max() <= 1e-8 * np.abs(a_ref).max(), np.abs(got - a_ref).max() / np.abs(a_ref).max()
    m_ref = m0 - np.linalg.solve(Mm, B @ a_ref.ravel())
    m_got = np.stack([pr["data"][k, 0].ravel()[cols] for k in range(3)]).ravel()  # (the float64 map; out.data is float32)
    assert np.abs(m_got - m_ref).max() <= 1e-8 * np.abs(m_ref).max()


def test_prior_limits(gpu_ctx):
    """A very large knee (s -> 0) gives the map and the offsets with hits of the destriper without a prior, to the CG
    tolerance; a very small knee forces each detector's offsets toward one constant."""
    from maria_amd.mappers import DestripingMapper

    tod, kw = _setup(seed=8)
    kw.update(noise_weights="uniform", tol=1e-11, max_iter=2000, baseline_length=0.32)
    plain = DestripingMapper([tod], **kw)
    ref = plain.run().data
    weak = DestripingMapper([tod], baseline_prior={"knee": 1e9}, **kw)
    got = weak.run().data
    assert weak.products["converged"]
    ok = np.isfinite(ref)
    np.testing.assert_array_equal(ok, np.isfinite(got))
    assert np.abs(got[ok] - ref[ok]).max() <= 1e-6 * np.abs(ref[ok]).max()
    hits = plain.products["hits"][0]
    a0, a1 = plain.products["baselines"][0], weak.products["baselines"][0]
    seen = hits > 0
    assert np.abs(a1[seen] - a0[seen]).max() <= 1e-6 * np.abs(a0).max()
    stiff = DestripingMapper([tod], baseline_prior={"knee": 1e-7}, **kw)
    stiff.run()
    a2 = stiff.products["baselines"][0]
    spread = lambda a: float(np.abs(a - a.mean(axis=1, keepdims=True)).max())  # noqa: E731
    assert spread(a2) <= 1e-4 * spread(a0), (spread(a2), spread(a0))


def test_prior_pays_on_the_1f_simulation(gpu_ctx, capsys):
    """The 1/f-dominated simulation of the destriper's front-end test (knee 20 Hz, 600 s, 50 Hz): with the simulator's own
    law as the prior (knee 20 Hz, alpha 1) 16-sample (0.32 s) baselines give a lower hits-weighted residual than no prior
    at 0.32 s and at 2 s.  Measured on an MI355X (noise seed 3): with the prior 1.796e-3 K_RJ, without 2.101e-3 (0.32 s)
    and 2.008e-3 (2 s), 1.12x below the better of the two; the bound is 1.08.  The CG took 69 iterations with the band
    preconditioner, 73 with the diagonal, 80 at 0.32 s without the prior.  The band preconditioner and the diagonal (band 0) give the same map to the CG tolerance."""
    from maria_amd.mappers import DestripingMapper

    tod, sky, centre, n, res = _front_end_1f()
    kw = dict(center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="IQU", nu=[150e9], frame="ra/dec",
              units="K_RJ", noise_weights="inverse_variance", tol=1e-8, max_iter=500)
    r = {}
    runs = (("prior 0.32 s", 0.32, {"knee": 20.0}), ("prior 0.32 s diagonal", 0.32, {"knee": 20.0, "band": 0}), ("plain 0.32 s", 0.32, None),
            ("plain 2 s", 2.0, None))
    for name, length, prior in runs:
        mapper = DestripingMapper([tod], baseline_length=length, baseline_prior=prior, **kw)
        out = mapper.run()
        assert mapper.products["converged"], name
        r[name] = (_residual_rms(mapper, out, sky), mapper.products["n_iter"])
    with capsys.disabled():
        print("\n1/f simulation, residual rms (K_RJ) and CG iterations: " + ", ".join(f"{k} {v[0]:.4e} ({v[1]})" for k, v in r.items()))
    assert abs(r["prior 0.32 s"][0] - r["prior 0.32 s diagonal"][0]) <= 1e-4 * r["prior 0.32 s"][0]
    best_plain = min(r["plain 0.32 s"][0], r["plain 2 s"][0])
    assert r["prior 0.32 s"][0] * PAYS_BOUND <= best_plain, r


PAYS_BOUND = 1.08
