"""The maximum-likelihood map-maker's operators (mrx_map_project, mrx_map_normal_apply, mrx_bin_map_blocks,
mrx_map_block_solve) against a scipy.sparse pointing matrix built from the oracle's restatement of the reference's
pointing (oracle.mapsample), and MaximumLikelihoodMapper end to end."""

import ctypes as C
import logging

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=[0, 1], ids=["composed", "chain"])
def pointing_mode(request, gpu_ctx):
    """Both forms of the pointing: the composed float64 rotation (default) and the float32 chain (MRX_OPT_POINTING_CHAIN)."""
    gpu_ctx.set_option(0, request.param)
    yield request.param
    gpu_ctx.set_option(0, 0)


def _t(a, dtype):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype)).to(DEV)


class Problem:
    """A daisy scan, a focal plane, a grid over 80 % of the scanned patch, two channels; the device inputs and the
    oracle's sparse P ([D T] x [S C n_eta n_xi])."""

    def __init__(self, D=37, T=3301, n=(12, 16), S=3, bilinear=False, frame="sky", seed=0, gamma=None):
        from maria_amd import synthetic
        from oracle import hotpath, mapsample

        rng = np.random.default_rng(seed)
        t = 1.7e9 + np.arange(T) / 50.0
        az, el = synthetic.daisy_scan(t)
        self.az, self.el = az.astype(np.float32), el.astype(np.float32)
        self.off = synthetic.hex_pack(D, np.radians(0.5))
        self.transform = None
        if frame == "sky":
            tilt = np.radians(35.0)
            Rx = np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]])
            w = 7.292e-5 * (t - t[0]) + 0.3
            Rz = np.zeros((T, 3, 3))
            Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(w), -np.sin(w), np.sin(w), np.cos(w), 1
            self.transform = Rx[None] @ Rz
        az_d, el_d = hotpath.broadcast(self.off, self.az, self.el)
        phi, theta = mapsample.frame_angles(az_d, el_d, self.transform)
        xyz = mapsample.phi_theta_to_xyz(phi[0], theta[0]).astype(float).mean(axis=0)
        xyz /= np.linalg.norm(xyz)
        self.centre = (float(np.arctan2(xyz[1], xyz[0]) % (2 * np.pi)), float(np.arcsin(xyz[2])))
        ox = mapsample.phi_theta_to_offsets(phi, theta, *self.centre)
        self.n_eta, self.n_xi = n
        he, hx = 0.8 * float(np.abs(ox[..., 1]).max()), 0.8 * float(np.abs(ox[..., 0]).max())
        self.eta, self.xi = np.linspace(he, -he, self.n_eta), np.linspace(-hx, hx, self.n_xi)
        self.S, self.Cn, self.D, self.T, self.bilinear = S, 2, D, T, bilinear
        if gamma is None:
            gamma = np.where(np.arange(D) % 5 == 0, np.nan, rng.uniform(0, np.pi, D))
        self.sw = mapsample.mueller_row(gamma)[:, :S]
        self.chan = (np.arange(D) % 2).astype(np.int32)
        _, pix, wts, n_pix, _ = mapsample.pointing_matrix_ingredients((ox[..., 1], ox[..., 0]), (self.eta, self.xi), bilinear)
        self.n_pix = n_pix
        rows = np.broadcast_to(np.arange(D * T).reshape(D, T), pix.shape)
        r, c, v = [], [], []
        for s in range(S):
            col = (s * self.Cn + self.chan[None, :, None]) * n_pix + pix
            r.append(rows.ravel()), c.append(col.ravel()), v.append((wts * self.sw[None, :, s, None]).ravel())
        self.P = scipy.sparse.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(D * T, S * self.Cn * n_pix))
        f32 = lambda a: _t(a, np.float32)  # noqa: E731
        self.d = dict(az=f32(self.az), el=f32(self.el), dx=f32(self.off[:, 0]), dy=f32(self.off[:, 1]), sw=_t(self.sw, np.float64),
                      chan=_t(self.chan, np.int32), tr=None if self.transform is None else _t(self.transform.reshape(-1, 9), np.float64))

    @property
    def tol(self):
        """nearest pixel: float64 rounding; bilinear: corner weights move by the float32 rounding of the offsets (6e-7 rad,
        the bound test_gpu_map holds the binning to) over a pixel"""
        return 4 * 6e-7 / min(abs(self.eta[1] - self.eta[0]), abs(self.xi[1] - self.xi[0])) if self.bilinear else 1e-9

    @property
    def map_shape(self):
        return (self.S, self.Cn, self.n_eta, self.n_xi)

    def sky(self):
        from maria_amd._lib import MrxSkyMap

        return MrxSkyMap(None, self.Cn, self.S, self.n_eta, self.n_xi, float(self.eta[0]), float(self.eta[1] - self.eta[0]),
                         float(self.xi[0]), float(self.xi[1] - self.xi[0]), self.centre[0], self.centre[1], int(self.bilinear), 0)

    def point(self):
        from maria_amd._lib import ptr

        d = self.d
        return (ptr(d["az"]), ptr(d["el"]), self.T, ptr(d["tr"]), ptr(d["dx"]), ptr(d["dy"]), ptr(d["sw"]), ptr(d["chan"]), self.D)

    def smooth_map(self, seed=1):
        rng = np.random.default_rng(seed)
        E, X = np.meshgrid(np.linspace(-1, 1, self.n_eta), np.linspace(-1, 1, self.n_xi), indexing="ij")
        m = np.zeros(self.map_shape)
        for s in range(self.S):
            for c in range(self.Cn):
                a, b = rng.uniform(-0.5, 0.5, 2)
                m[s, c] = (1.0 - 0.3 * s + 0.2 * c) * np.exp(-((E - a) ** 2 + (X - b) ** 2)) + 0.1 * rng.normal()
        return m

    def project(self, ctx, x, alpha=1.0, beta=0.0, out=None):
        import torch

        from maria_amd._lib import ptr

        out = torch.full((self.D, self.T), float("nan"), dtype=torch.float32, device=DEV) if out is None else out
        ctx.call("mrx_map_project", C.byref(self.sky()), ptr(x), *self.point(), alpha, beta, ptr(out), out.stride(0))
        return out

    def normal(self, ctx, x, weight=None, det_w=None, work="full"):
        import torch

        from maria_amd._lib import ptr

        sky = self.sky()
        lo, full = C.c_size_t(), C.c_size_t()
        assert ctx.lib.mrx_map_normal_work_bytes(C.byref(sky), self.D, self.T, C.byref(lo), C.byref(full)) == 0
        buf = None if work is None else torch.empty(full.value if work == "full" else lo.value, dtype=torch.uint8, device=DEV)
        y = torch.zeros(self.map_shape, dtype=torch.float64, device=DEV)
        ctx.call("mrx_map_normal_apply", C.byref(sky), ptr(x), ptr(weight), 0 if weight is None else weight.stride(0), ptr(det_w),
                 *self.point(), ptr(y), ptr(buf), 0 if buf is None else buf.numel())
        return y.cpu().numpy()

    def blocks(self, ctx, weight=None, det_w=None):
        import torch

        from maria_amd._lib import ptr

        H = torch.zeros((self.S * (self.S + 1) // 2, self.Cn, self.n_eta, self.n_xi), dtype=torch.float64, device=DEV)
        ctx.call("mrx_bin_map_blocks", C.byref(self.sky()), ptr(weight), 0 if weight is None else weight.stride(0), ptr(det_w),
                 *self.point(), ptr(H))
        return H


def _flip_tolerant_close(got, ref, rtol, max_bad_frac):
    """Equal to rtol of the largest value except on a few entries (nearest pixel: samples within float32 rounding of a
    pixel edge may take the neighbouring pixel in one implementation and not the other)."""
    bad = np.abs(got - ref) > rtol * np.abs(ref).max()
    assert bad.mean() <= max_bad_frac, (bad.mean(), np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("frame", ["sky", "az/el"])
def test_project_matches_the_sparse_pointing_matrix(gpu_ctx, bilinear, S, frame, pointing_mode):
    """mrx_map_project = P_sparse @ x to float32 rounding; alpha / beta, and beta = 0 over a NaN-filled output."""
    pb = Problem(S=S, bilinear=bilinear, frame=frame, T=2051)
    x = pb.smooth_map()
    ref = (pb.P @ x.ravel()).reshape(pb.D, pb.T)
    d_x = _t(x, np.float64)
    out = pb.project(gpu_ctx, d_x)  # over NaN: beta = 0 does not read it
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    # bilinear: weights move by float32 rounding of the offsets (<= 6e-7 rad of a pixel) -- no sample disagrees beyond that
    _flip_tolerant_close(got, ref, pb.tol if bilinear else 2e-6, 0.0 if bilinear else 2e-3)
    out2 = pb.project(gpu_ctx, d_x, alpha=2.0, beta=-0.5, out=out.clone())
    np.testing.assert_allclose(out2.cpu().numpy(), (1.5 * got).astype(np.float32), rtol=1e-6, atol=1e-7 * np.abs(got).max())


@pytest.mark.parametrize("bilinear", [False, True])
def test_project_is_the_adjoint_of_the_binning(gpu_ctx, bilinear, pointing_mode):
    """<P x, W y> = <x, P^T W y> with P^T W y from the shipped mrx_bin_map (d_sum): ties the new operator to the binning."""
    import torch

    from maria_amd._lib import ptr

    pb = Problem(S=3, bilinear=bilinear, T=2051)
    rng = np.random.default_rng(4)
    x = pb.smooth_map()
    y = rng.normal(size=(pb.D, pb.T)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, (pb.D, pb.T)).astype(np.float32)
    px = pb.project(gpu_ctx, _t(x, np.float64)).cpu().numpy().astype(np.float64)
    msum = torch.zeros(pb.map_shape, dtype=torch.float64, device=DEV)
    mwgt = torch.zeros_like(msum)
    d_y, d_w = _t(y, np.float32), _t(w, np.float32)
    gpu_ctx.call("mrx_bin_map", C.byref(pb.sky()), ptr(d_y), d_y.stride(0), ptr(d_w), d_w.stride(0), *pb.point(), ptr(msum), ptr(mwgt))
    lhs = float(np.sum(px * w.astype(np.float64) * y))
    rhs = float(np.sum(x * msum.cpu().numpy()))
    assert abs(lhs - rhs) <= 1e-6 * np.sum(np.abs(px * w * y)), (lhs, rhs)


@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("shape", [(12, 16), (70, 150)])
def test_normal_operator(gpu_ctx, bilinear, shape, pointing_mode):
    """mrx_map_normal_apply = P^T W P x: the routed form (whole buffer and the minimum, chunked) and the atomic form agree
    to float64 rounding; against the sparse P (up to the samples near a pixel edge); per-sample and per-detector weights."""
    pb = Problem(S=3, bilinear=bilinear, n=shape, T=3301)
    rng = np.random.default_rng(5)
    x = pb.smooth_map()
    d_x = _t(x, np.float64)
    w = rng.uniform(0.5, 2.0, (pb.D, pb.T)).astype(np.float32)
    dw = rng.uniform(0.5, 3.0, pb.D)
    d_w, d_dw = _t(w, np.float32), _t(dw, np.float64)
    W = (w.astype(np.float64) * dw[:, None]).ravel()
    ref = (pb.P.T @ (W * (pb.P @ x.ravel()))).reshape(pb.map_shape)
    routed = pb.normal(gpu_ctx, d_x, d_w, d_dw, work="full")
    chunked = pb.normal(gpu_ctx, d_x, d_w, d_dw, work="min")
    atomic = pb.normal(gpu_ctx, d_x, d_w, d_dw, work=None)
    scale = np.abs(atomic).max()
    assert scale > 0
    # float64 rounding; with the float32 chain and bilinear weights the two kernels' offsets may differ by a float32 ulp (so
    # do mrx_bin_map's and mrx_bin_map_bucketed's there), which moves a corner weight by the oracle tolerance at most
    agree = pb.tol if (pointing_mode and bilinear) else 1e-12
    assert np.abs(routed - atomic).max() <= agree * scale and np.abs(chunked - atomic).max() <= agree * scale
    assert np.abs(routed - chunked).max() <= 1e-12 * scale
    _flip_tolerant_close(routed, ref, pb.tol, 0.1 if not bilinear else 0.0)
    assert np.abs(routed - ref).sum() <= 2e-3 * np.abs(ref).sum()
    # each weight alone
    only_dw = pb.normal(gpu_ctx, d_x, None, d_dw)
    ref_dw = (pb.P.T @ (np.repeat(dw, pb.T) * (pb.P @ x.ravel()))).reshape(pb.map_shape)
    _flip_tolerant_close(only_dw, ref_dw, pb.tol, 0.1 if not bilinear else 0.0)
    only_w = pb.normal(gpu_ctx, d_x, d_w, None)
    ref_w = (pb.P.T @ (w.astype(np.float64).ravel() * (pb.P @ x.ravel()))).reshape(pb.map_shape)
    _flip_tolerant_close(only_w, ref_w, pb.tol, 0.1 if not bilinear else 0.0)


@pytest.mark.parametrize("bilinear", [False, True])
def test_blocks_and_block_solve(gpu_ctx, bilinear):
    """mrx_bin_map_blocks = the block diagonal of P^T W P (both forms of the pointing: the float32 chain and the composed
    rotation); mrx_map_block_solve = H^-1 r per pixel, NaN exactly where the block's reciprocal condition number is below
    rcond (or the pixel has no hits), 0 there in the preconditioner's form."""
    import torch

    from maria_amd._lib import ptr

    pb = Problem(S=3, bilinear=bilinear, n=(12, 16), T=2051)
    rng = np.random.default_rng(7)
    w = rng.uniform(0.5, 2.0, (pb.D, pb.T)).astype(np.float32)
    dw = rng.uniform(0.5, 3.0, pb.D)
    W = (w.astype(np.float64) * dw[:, None]).ravel()
    full = (pb.P.T @ scipy.sparse.diags(W) @ pb.P).tocsr()
    n, Cn = pb.n_pix, pb.Cn
    ref = np.zeros((6, Cn, pb.n_eta, pb.n_xi))  # H[k, l], k <= l
    idx = 0
    for k in range(3):
        for l in range(k, 3):
            for c in range(Cn):
                rows, cols = (k * Cn + c) * n + np.arange(n), (l * Cn + c) * n + np.arange(n)
                ref[idx, c] = np.asarray(full[rows, cols]).reshape(pb.n_eta, pb.n_xi)
            idx += 1
    for chain in (1, 0):  # the float32 chain (MRX_OPT_POINTING_CHAIN), then the composed rotation (the default)
        gpu_ctx.set_option(0, chain)
        try:
            H = pb.blocks(gpu_ctx, _t(w, np.float32), _t(dw, np.float64))
        finally:
            gpu_ctx.set_option(0, 0)
        got = H.cpu().numpy()
        assert got.shape == ref.shape
        _flip_tolerant_close(got, ref, pb.tol, 0.1 if not bilinear else 0.0)
    # a pixel never seen, and one seen by a single detector angle: singular blocks
    Hn = got.copy()
    Hn[:, 0, 0, 0] = 0.0
    wv = np.array([1.0, 0.6, 0.8])
    Hn[:, 1, 0, 0] = [wv[0] * wv[0], wv[0] * wv[1], wv[0] * wv[2], wv[1] * wv[1], wv[1] * wv[2], wv[2] * wv[2]]
    r = rng.normal(size=pb.map_shape)
    d_H, d_r = _t(Hn, np.float64), _t(r, np.float64)
    z = torch.empty_like(d_r)
    mask = torch.empty((Cn, pb.n_eta, pb.n_xi), dtype=torch.uint8, device=DEV)
    rcond = 1e-3
    gpu_ctx.call("mrx_map_block_solve", 3, Cn, n, ptr(d_H), ptr(d_r), rcond, 1, ptr(z), ptr(mask))
    z, mask = z.cpu().numpy(), mask.cpu().numpy().astype(bool)
    expect = np.zeros((Cn, pb.n_eta, pb.n_xi), bool)
    for c in range(Cn):
        for e in range(pb.n_eta):
            for xx in range(pb.n_xi):
                h = Hn[:, c, e, xx]
                A = np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])
                if h[0] <= 0 or np.linalg.det(A) <= 0:
                    continue
                rc = 1.0 / (np.linalg.norm(A, 1) * np.linalg.norm(np.linalg.inv(A), 1))
                expect[c, e, xx] = rc >= rcond
                if expect[c, e, xx]:
                    np.testing.assert_allclose(z[:, c, e, xx], np.linalg.solve(A, r[:, c, e, xx]), rtol=1e-9, atol=1e-12)
    assert not expect[0, 0, 0] and not expect[1, 0, 0] and expect.mean() > 0.3 and (~expect).any()
    np.testing.assert_array_equal(mask, expect)
    assert np.isnan(z[:, ~expect]).all() and np.isfinite(z[:, expect]).all()
    z0 = torch.empty_like(d_r)
    gpu_ctx.call("mrx_map_block_solve", 3, Cn, n, ptr(d_H), ptr(d_r), rcond, 0, ptr(z0), None)
    assert (z0.cpu().numpy()[:, ~expect] == 0).all()


# ---- MaximumLikelihoodMapper ----

def _tods(D=48, T=6000, angles=(0.0, 45.0, 90.0, 135.0), bands=((150e9, "f150"),), seed=0, fov=0.4):
    """TODs (az/el frame) of a focal plane whose detectors take the given polarisation angles in turn, one per band."""
    from maria_amd import synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    t = 1.7e9 + np.arange(T) / 50.0
    az, el = synthetic.daisy_scan(t, radius_deg=0.3)
    pos = synthetic.hex_pack(D, np.radians(fov))
    bl = [Band(center=c, width=0.2 * c, name=n) for c, n in bands]
    nb = len(bl)
    gamma = np.tile(np.radians(np.asarray(angles))[np.arange(D) % len(angles)], nb)
    dets = Detectors(np.tile(pos, (nb, 1)), bl, np.repeat(np.arange(nb), D), gamma=gamma)
    coords = Coordinates(t, az, el, offsets=dets.offsets)
    return TOD({"map": np.zeros((dets.n, T), np.float32)}, dets, coords, units="K_RJ"), float(np.degrees(az.mean())), float(np.degrees(el.mean()))


def _fill_with_projection(mapper, tods, m_true):
    """TOD = P m_true through mrx_map_project with exactly the mapper's inputs."""
    import torch

    from maria_amd._lib import Context, ptr

    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    sky = mapper._sky()
    x = _t(m_true, np.float64)
    for tod in tods:
        signal, weight, az, el, tr, dx, dy, sw, chan = mapper._tod_inputs(tod, ctx, unit_i_response=mapper.units == "K_RJ")
        out = torch.empty_like(signal)
        ctx.call("mrx_map_project", C.byref(sky), ptr(x), ptr(az), ptr(el), signal.shape[1], ptr(tr), ptr(dx), ptr(dy), ptr(sw), ptr(chan),
                 signal.shape[0], 1.0, 0.0, ptr(out), out.stride(0))
        tod.data = {"map": out.cpu().numpy()}
    torch.cuda.synchronize()


def _iqu_map(mapper, seed=3):
    rng = np.random.default_rng(seed)
    S, Cn = len(mapper.stokes), len(mapper.nu)
    E, X = np.meshgrid(np.linspace(-1, 1, mapper.n_eta), np.linspace(-1, 1, mapper.n_xi), indexing="ij")
    m = np.zeros((S, Cn, mapper.n_eta, mapper.n_xi))
    for s in range(S):
        for c in range(Cn):
            a, b = rng.uniform(-0.4, 0.4, 2)
            m[s, c] = (1.0 if s == 0 else 0.3 * (-1) ** s) * np.exp(-((E - a) ** 2 + (X - b) ** 2) / 0.3) + 0.05 * rng.normal(size=E.shape)
    return m


def test_nearest_polarised_recovery(gpu_ctx):
    """Detectors at 0, 45, 90 and 135 degrees, TOD = P m_true of an IQU map: the block solve returns I, Q and U to
    float32 rounding on the solved pixels; pixels seen at one angle only are NaN; BinMapper does not recover Q / U."""
    from maria_amd.mappers import BinMapper, MaximumLikelihoodMapper

    tod, caz, cel = _tods()
    kw = dict(center=(caz, cel), width=0.8, resolution=0.8 / 40, stokes="IQU", nu=150e9, frame="az/el", units="K_RJ")
    mapper = MaximumLikelihoodMapper([tod], noise_weights="uniform", **kw)
    m_true = _iqu_map(mapper)
    _fill_with_projection(mapper, [tod], m_true)
    out = mapper.run()
    assert out.data.shape == m_true.shape and out.data.dtype == np.float32
    solved = np.isfinite(out.data[0, 0])
    assert solved.mean() > 0.2 and mapper.products["converged"] and mapper.products["n_iter"] == 0
    assert np.all(np.isfinite(out.data[:, 0][:, solved])) and np.all(np.isnan(out.data[:, 0][:, ~solved]))
    err = np.abs(mapper.products["data"][:, 0][:, solved] - m_true[:, 0][:, solved]).max(axis=1) / np.abs(m_true[:, 0][:, solved]).max(axis=1)
    assert np.all(err <= 1e-5), err
    np.testing.assert_array_equal(out.weight, mapper.products["blocks"][:1])
    # hit pixels the solve left out are exactly the singular ones (their hits all at one angle pair)
    hit = mapper.products["blocks"][0, 0] > 0
    left = hit & ~solved
    H = mapper.products["blocks"][:, 0]
    for e, x in zip(*np.nonzero(left)):
        h = H[:, e, x]
        A = np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])
        sv = np.linalg.svd(A, compute_uv=False)
        assert sv[-1] <= 3e-3 * sv[0], sv
    # the binned map mixes I into Q and U and scales them: it does not recover them
    binned = BinMapper([tod], **kw).run().data
    qerr = np.nanmax(np.abs(binned[1:, 0][:, solved] - m_true[1:, 0][:, solved])) / np.abs(m_true[1:, 0][:, solved]).max()
    assert qerr > 0.1, qerr


def test_one_angle_pixels_are_nan(gpu_ctx):
    """Every detector at the same angle: no pixel's IQU block is invertible, the whole map is NaN; with stokes='I' the
    same TOD solves."""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, caz, cel = _tods(angles=(30.0,))
    kw = dict(center=(caz, cel), width=0.8, resolution=0.8 / 40, nu=150e9, frame="az/el", units="K_RJ", noise_weights="uniform")
    mapper = MaximumLikelihoodMapper([tod], stokes="IQU", **kw)
    _fill_with_projection(mapper, [tod], _iqu_map(mapper))
    assert np.isnan(mapper.run().data).all()
    assert np.isfinite(MaximumLikelihoodMapper([tod], stokes="I", **kw).run().data).any()


def test_bilinear_cg_matches_spsolve(gpu_ctx, caplog):
    """Bilinear pointing: PCG on P^T W P against scipy's direct solve on the solved pixels; the recorded residuals fall
    below tol; with max_iter=2 the run ends unconverged, with a warning and no exception."""
    import torch

    from maria_amd._lib import Context
    from maria_amd.mappers import MaximumLikelihoodMapper
    from oracle import mapsample

    tod, caz, cel = _tods(D=20, T=20000, fov=0.3)
    kw = dict(center=(caz, cel), width=0.64, resolution=0.01, stokes="IQU", nu=150e9, frame="az/el", units="K_RJ", bilinear=True,
              noise_weights="uniform")
    mapper = MaximumLikelihoodMapper([tod], tol=1e-8, max_iter=200, **kw)
    assert (mapper.n_eta, mapper.n_xi) == (64, 64)
    m_true = _iqu_map(mapper)
    _fill_with_projection(mapper, [tod], m_true)
    rng = np.random.default_rng(9)
    tod.data["map"] = tod.data["map"] + (0.01 * rng.normal(size=tod.data["map"].shape)).astype(np.float32)  # not exactly in the range of P
    out = mapper.run()
    res = mapper.products["residuals"]
    assert mapper.products["converged"] and res[-1] < 1e-8 and len(res) == mapper.products["n_iter"] + 1
    # the oracle: sparse P from the same pointing restatement, restricted to the solved pixels
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    coords = tod.coords
    from oracle import hotpath

    az_d, el_d = hotpath.broadcast(coords.offsets, coords._baz.astype(np.float32), coords._bel.astype(np.float32))
    ox = mapsample.phi_theta_to_offsets(az_d, el_d, *mapper.center)
    _, pix, wts, n_pix, _ = mapsample.pointing_matrix_ingredients((ox[..., 1], ox[..., 0]), (mapper.eta, mapper.xi), True)
    sw = mapsample.mueller_row(tod.dets.gamma)[:, :3]
    sw = sw / sw[:, :1]  # (K_RJ: unit response to I)
    D, T = tod.data["map"].shape
    rows = np.broadcast_to(np.arange(D * T).reshape(D, T), pix.shape).ravel()
    P = scipy.sparse.hstack([scipy.sparse.csr_matrix(((wts * sw[None, :, s, None]).ravel(), (rows, pix.ravel())), shape=(D * T, n_pix))
                             for s in range(3)]).tocsr()
    solved = np.isfinite(out.data[0, 0]).ravel()
    keep = np.tile(solved, 3)
    Ps = P[:, keep]
    ref = scipy.sparse.linalg.spsolve((Ps.T @ Ps).tocsc(), Ps.T @ tod.data["map"].astype(np.float64).ravel())
    got = mapper.products["data"][:, 0].reshape(3, -1)[:, solved].ravel()
    assert solved.mean() > 0.3
    # (the oracle's pointing is the reference's float32 chain restated: corner weights differ by float32 rounding, which the
    # solve amplifies by the conditioning of P^T P on the sparsely hit pixels)
    assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
    short = MaximumLikelihoodMapper([tod], tol=1e-8, max_iter=2, **kw)
    with caplog.at_level(logging.WARNING, logger="maria"):
        short.run()
    assert short.products["converged"] is False and short.products["n_iter"] == 2
    assert any("conjugate gradients" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("bilinear", [False, True])
def test_several_tods_give_the_map_of_one(gpu_ctx, bilinear):
    """Two TODs (halves of the focal plane) give the map of one TOD holding all their rows."""
    from maria_amd.mappers import MaximumLikelihoodMapper
    from maria_amd.sim import TOD, Coordinates

    tod, caz, cel = _tods(D=40, T=8000)
    kw = dict(center=(caz, cel), width=0.8, resolution=0.8 / 40, stokes="IQU", nu=150e9, frame="az/el", units="K_RJ", bilinear=bilinear,
              noise_weights="inverse_variance", tol=1e-10, max_iter=300)
    one = MaximumLikelihoodMapper([tod], **kw)
    _fill_with_projection(one, [tod], _iqu_map(one))
    tod.data["map"] = tod.data["map"] + (0.01 * np.random.default_rng(2).normal(size=tod.data["map"].shape)).astype(np.float32)
    halves = []
    for idx in (np.arange(0, 40, 2), np.arange(1, 40, 2)):
        dets = tod.dets.subset(idx)
        halves.append(TOD({"map": tod.data["map"][idx]}, dets, Coordinates(tod.coords.t, tod.coords._baz, tod.coords._bel, offsets=dets.offsets),
                          units="K_RJ"))
    a = one.run().data
    two = MaximumLikelihoodMapper(halves, **kw)
    b = two.run().data
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    ok = np.isfinite(a)
    assert ok.any() and np.abs(a[ok] - b[ok]).max() <= 1e-6 * np.abs(a[ok]).max()


def _front_end(noise):
    from maria_amd import map as mmap
    from maria_amd.instrument import Band, Detectors, Instrument, Site
    from maria_amd.sim import Plan, Simulation, sky_transform_stack
    from oracle import mapsample

    bands = [Band(center=90e9, width=30e9, name="f090", NEP=3e-17, knee=1.0), Band(center=150e9, width=40e9, name="f150", NEP=4e-17, knee=1.0)]
    from maria_amd import synthetic

    npos, width = 150, 1.0
    pos = synthetic.hex_pack(npos, np.radians(width / 2))
    gamma = np.tile(np.radians([0.0, 45.0, 90.0, 135.0])[np.arange(npos) % 4], 2)
    dets = Detectors(np.tile(pos, (2, 1)), bands, np.repeat([0, 1], npos), primary_size=1000.0, gamma=gamma)
    plan = Plan.daisy(start_time=1.7e9, duration=60.0, sample_rate=50.0, scan_center=(120.0, 55.0), radius=width / 3, speed=0.5)
    site = Site(altitude=5190.0)
    transform = sky_transform_stack(plan.time, site.latitude, site.longitude)
    phi, theta = mapsample.frame_angles(plan.phi.astype(np.float32)[None], plan.theta.astype(np.float32)[None], transform)
    xyz = mapsample.phi_theta_to_xyz(phi[0], theta[0]).astype(float).mean(axis=0)
    xyz /= np.linalg.norm(xyz)
    centre = (float(np.arctan2(xyz[1], xyz[0]) % (2 * np.pi)), float(np.arcsin(xyz[2])))
    n = 64
    res = width / (n - 1)
    X, Y = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    blob = -5e-3 * (1 + ((X - 0.1) ** 2 + (Y + 0.05) ** 2) / 0.04) ** -1.0
    data = np.stack([np.stack([(1 + 0.3 * c) * s * blob for c in range(2)]) for s in (1.0, 0.2, -0.1)]).astype(np.float32)
    sky = mmap.ProjectionMap(data, nu=[90e9, 150e9], stokes="IQU", width=width, center=np.degrees(centre), frame="ra/dec")
    sim = Simulation(Instrument(dets), plan, site, map=sky, noise=noise, noise_seed=3)
    (tod,) = sim.run()
    return tod, sky, centre, n, res


def test_front_end_recovers_an_iqu_map(gpu_ctx):
    """Simulation(map=IQU, two channels) in K_RJ with polarised detectors at four angles per band, then the mapper on the
    input's grid: the hit-weighted rms of (recovered - input) over the solved pixels is below 1e-3 K_RJ per plane and
    channel (the reference's assertion for its map round trip), and the recovered Q and U follow the input's."""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, sky, centre, n, res = _front_end(noise=False)
    assert tod.units == "K_RJ"
    mapper = MaximumLikelihoodMapper([tod], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="IQU",
                                     nu=[90e9, 150e9], frame="ra/dec", units="K_RJ", noise_weights="uniform")
    out = mapper.run()
    assert out.data.shape == sky.data.shape and np.allclose(out.xi, sky.xi, atol=1e-12)
    solved = np.isfinite(out.data)
    assert solved[0].mean() > 0.3
    w = np.where(solved[0], mapper.products["weight"][0], 0.0)  # H[0, 0]: the hits, as the reference weighs its residual
    for s in range(3):
        for c in range(2):
            ok = solved[s, c]
            rms = np.sqrt(np.sum(w[c][ok] * (out.data[s, c][ok] - sky.data[s, c][ok]) ** 2) / np.sum(w[c][ok]))
            assert rms < 1e-3, (s, c, rms)
            if s:
                assert np.corrcoef(out.data[s, c][ok], sky.data[s, c][ok])[0, 1] > 0.9, (s, c)


def test_front_end_with_noise_and_inverse_variance_weights(gpu_ctx):
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, sky, centre, n, res = _front_end(noise=True)
    mapper = MaximumLikelihoodMapper([tod], center=np.degrees(centre), width=(n + 0.5) * res, resolution=res, stokes="IQU",
                                     nu=[90e9, 150e9], frame="ra/dec", units="K_RJ", noise_weights="inverse_variance")
    out = mapper.run()
    solved = np.isfinite(out.data)
    assert solved.mean() > 0.3 and np.isfinite(out.data[solved]).all()
