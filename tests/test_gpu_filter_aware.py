"""The filter-aware maximum-likelihood map: mrx_sosfilt_transpose and mrx_tod_detrend_window_transpose
against the float64 restatement of tests/filter_aware_ref.py, the pre-processing operator F and F^T of
maria_amd.tod_processing against it and against process_tod, and MaximumLikelihoodMapper(filter_aware=True) against dense
float64 solves of (P^T F^T W F P) m = P^T F^T W F d, against the plain map on extended emission, and its default."""

import ctypes as C

import numpy as np
import pytest
import scipy.signal

import filter_aware_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MRX_ERR_INVALID = -1
STEP_TOL = 3e-7  # per row and float32-rounded step: the forward kernels' bound (test_gpu_todproc_kernels._worst_row)


# ---- 1, 2: the two kernels ----------------------------------------------------------------------

def _ref_sosfilt_transpose(sos, x, remove_slope):
    u = scipy.signal.sosfilt(sos, x.astype(np.float64)[:, ::-1], axis=-1)[:, ::-1]
    return ref.slope_transpose(u) if remove_slope else u


def _run_transpose(ctx, sos, M, x, remove_slope, layout):
    """mrx_sosfilt_transpose of x [D, T] in one of test_gpu_todproc_kernels._run_sosfilt's four layouts; checks the
    padding and, out of place, the input; returns the result [D, T]."""
    import test_gpu_todproc_kernels as k
    from maria_amd._lib import ptr

    D, T = x.shape
    r4 = -(-T // 4) * 4
    ld_in, ld_out, off = {"inplace": (T + 3, T + 3, 0), "out": (r4 + 4, r4 + 8, 0), "off1": (T + 1, T + 5, 1),
                          "off4": (r4 + 4, r4 + 12, 4)}[layout]
    fin, vin = k._buffer(D, T, ld_in, off, x)
    fout, vout = (fin, vin) if layout == "inplace" else k._buffer(D, T, ld_out, off)
    work = k._work(ctx, D, T, len(sos))
    rc = ctx.lib.mrx_sosfilt_transpose(ctx.handle, sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos), ptr(M), ptr(vin), ld_in, D, T,
                                       remove_slope, ptr(vout), ld_out, ptr(work))
    assert rc == 0
    got = vout[:, :T].cpu().numpy()
    assert k._untouched(fout, D, T, ld_out, off), "mrx_sosfilt_transpose wrote outside [D, T]"
    if layout != "inplace":
        assert k._untouched(fin, D, T, ld_in, off) and np.array_equal(vin[:, :T].cpu().numpy(), x), "the input changed"
    return got


# Bessel order o is o + 1 sections: 1, 4 and 8 sections of a low pass, of a high pass, and of both (a low + high cascade
# has at least two sections: 2, 4 and 8)
TRANSPOSE_CASCADES = [("low", 0), ("low", 3), ("low", 7), ("high", 0), ("high", 3), ("high", 7),
                      (("low", 0), ("high", 0)), (("low", 1), ("high", 1)), (("low", 3), ("high", 3))]


@pytest.mark.parametrize("cascade", TRANSPOSE_CASCADES, ids=lambda c: str(c).replace(" ", ""))
def test_sosfilt_transpose_matches_the_reference(gpu_ctx, cascade):
    """out = [S^T] J H J in against scipy on the reversed row (and the two float64 sums of S^T), every T around the
    chunk (256) and the workgroup (65 536), the four layouts, with and without remove_slope: per row
    max |got - ref| <= 3e-7 max |ref_row|, the forward kernel's bound.

    Measured on an MI355X: worst row 5.2e-8 .. 5.9e-8 of max |ref_row| for all nine cascades.  The two sums of S^T are
    taken as <H a, in> and <H b, in> with serially filtered H a and H b: summing the time-parallel outputs themselves
    missed this bound for the 4-section low + high cascade at T = 65 537 (end sample off by 1.05e-5 against 1.57e-6),
    the chained states' 1e-9 rounding being of one sign over the row.  At T = 1 the reference is exactly
    zero (S = 0 on one sample) and so must the result be."""
    import test_gpu_todproc_kernels as k

    sos = k._cascade(cascade)
    M = k._chunk_matrix(gpu_ctx, sos)
    worst = 0.0
    for T in (1, 5, 255, 256, 257, 700, 65_537):
        x = k._rows(3 if T > 60_000 else 7, T, seed=T + len(sos))
        for remove_slope in (0, 1):
            want = _ref_sosfilt_transpose(sos, x, remove_slope)
            for layout in ("inplace", "out", "off1", "off4"):
                got = _run_transpose(gpu_ctx, sos, M, x, remove_slope, layout)
                worst = max(worst, k._worst_row(got, want, STEP_TOL))
    print(f"[filter-aware] sosfilt transpose {cascade} S={len(sos)}: worst row err {worst:.2e} max|ref_row|")


def test_sosfilt_transpose_is_the_forward_calls_adjoint(gpu_ctx):
    """<H S x, y> = <x, S^T H^T y> between the two device calls on a row of several workgroups."""
    import test_gpu_todproc_kernels as k

    sos = k._cascade((("low", 1), ("high", 1)))
    M = k._chunk_matrix(gpu_ctx, sos)
    rng = np.random.default_rng(3)
    D, T = 4, 140_001
    x, y = (rng.normal(size=(D, T)).astype(np.float32) for _ in range(2))
    Fx = k._run_sosfilt(gpu_ctx, sos, x, 1, "out").astype(np.float64)
    Fty = _run_transpose(gpu_ctx, sos, M, y, 1, "out").astype(np.float64)
    gap = np.abs(np.sum(Fx * y, axis=1) - np.sum(x * Fty, axis=1))
    bound = STEP_TOL * (np.abs(Fx).max(axis=1) * np.abs(y).sum(axis=1) + np.abs(Fty).max(axis=1) * np.abs(x).sum(axis=1))
    print(f"[filter-aware] sosfilt adjoint gap / bound: {(gap / bound).max():.2e}")
    assert np.all(gap <= bound), gap / bound


@pytest.mark.parametrize("n_sections,D", [(0, 4), (9, 4), (4, 65_536)])
def test_sosfilt_transpose_refusals(gpu_ctx, n_sections, D):
    """What mrx_sosfilt refuses (0 or 9 sections, more rows than one launch): MRX_ERR_INVALID, nothing written."""
    import torch

    import test_gpu_todproc_kernels as k
    from maria_amd._lib import ptr

    T = 8
    sos = k._sos(("low", 3), ("high", 4)) if n_sections == 9 else k._sos(("low", 1), ("high", 1), ("low", 3))
    x = torch.ones(D, T, dtype=torch.float32, device=DEV)
    out = torch.full((D, T), k.SENTINEL, dtype=torch.float32, device=DEV)
    M = torch.zeros(18, 18, dtype=torch.float64, device=DEV)
    work = torch.zeros(2 * D + D * 18 + 16, dtype=torch.float64, device=DEV)
    args = (sos.ctypes.data_as(C.POINTER(C.c_double)), n_sections, ptr(M), ptr(x), T, D, T, 1, ptr(out), T, ptr(work))
    assert gpu_ctx.lib.mrx_sosfilt_transpose(gpu_ctx.handle, *args) == MRX_ERR_INVALID
    if n_sections == 4:  # the other refusals of the forward call: null pointers, a short leading dimension, negative sizes
        for bad in ((None, *args[1:]), (*args[:3], None, *args[4:]), (*args[:8], None, *args[9:]), (*args[:10], None),
                    (*args[:4], T - 1, 4, *args[6:]), (*args[:9], T - 1, args[10]), (*args[:5], -1, *args[6:])):
            assert gpu_ctx.lib.mrx_sosfilt_transpose(gpu_ctx.handle, *bad) == MRX_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == k.SENTINEL).all()) and bool((x == 1).all()) and bool((work == 0).all())


@pytest.mark.parametrize("flags", ["slope", "window", "slope+window"])
def test_detrend_window_transpose_matches_numpy(gpu_ctx, flags):
    """x = S^T diag(w) y in place against float64 numpy, every flag combination, D around nothing in particular (one
    workgroup per row), T = 1, 2, 3 and around the 256-sample stride, ld > T with sentinels in the padding; the bound of
    test 1."""
    import torch

    import test_gpu_todproc_kernels as k
    from maria_amd._lib import ptr

    slope, window = "slope" in flags, "window" in flags
    worst = 0.0
    for D in (1, 17, 300):
        for T in (1, 2, 3, 255, 256, 257, 4099):
            y = k._rows(D, T, seed=D * 10_000 + T)
            ld = T + 3
            flat, view = k._buffer(D, T, ld, 0, y)
            w = scipy.signal.windows.tukey(T, alpha=0.5) if window else None
            d_w = torch.as_tensor(w).to(DEV) if window else None
            gpu_ctx.call("mrx_tod_detrend_window_transpose", ptr(view), ld, D, T, int(slope), ptr(d_w))
            got = view[:, :T].cpu().numpy()
            assert k._untouched(flat, D, T, ld, 0), (D, T)
            u = y.astype(np.float64) * (w if window else 1.0)
            want = ref.slope_transpose(u) if slope else u
            worst = max(worst, k._worst_row(got, want, STEP_TOL))
            if not window:  # nothing but the two end samples moves
                assert np.array_equal(got[:, 1:-1], y[:, 1:-1])
    print(f"[filter-aware] detrend transpose {flags}: worst row err {worst:.2e} max|ref_row|")


def test_detrend_window_transpose_neither_flag_and_refusals(gpu_ctx):
    import torch

    import test_gpu_todproc_kernels as k
    from maria_amd._lib import ptr

    x = k._rows(17, 257, seed=1)
    flat, view = k._buffer(17, 257, 260, 0, x)
    before = flat.clone()
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    assert lib.mrx_tod_detrend_window_transpose(h, ptr(view), 260, 17, 257, 0, None) == 0
    assert lib.mrx_tod_detrend_window_transpose(h, None, 260, 17, 257, 1, None) == MRX_ERR_INVALID
    assert lib.mrx_tod_detrend_window_transpose(h, ptr(view), 256, 17, 257, 1, None) == MRX_ERR_INVALID
    assert lib.mrx_tod_detrend_window_transpose(h, ptr(view), 260, -1, 257, 1, None) == MRX_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(flat, before)


# ---- 3: the operator ----------------------------------------------------------------------------

FULL = {"remove_slope": {}, "remove_spline": {"knot_spacing": 15.0, "remove_el_gradient": True}, "window": {"name": "hann"},
        "filter": {"f_lower": 0.2, "f_upper": 10.0}, "remove_modes": {"modes_to_remove": 2}}
FULL_ROUNDED_STEPS = 5  # every step of FULL stores float32 once (the filter's slope is float64 inside mrx_sosfilt)


def _copy(config):
    return {k: dict(v) for k, v in config.items()}


def _chain(steps, x, transpose):
    """The float64 reference's result and, per row, the largest magnitude along the chain (the input's included): a
    float32-rounded step errs by at most STEP_TOL of the larger of what it reads and what it writes."""
    x = np.asarray(x, np.float64)
    top = np.abs(x).max(axis=1)
    for name, p in (reversed(steps) if transpose else steps):
        x = ref._step(name, p, x, transpose)
        top = np.maximum(top, np.abs(x).max(axis=1))
    return x, top


def test_operator_reproduces_process_tod_and_matches_the_reference(gpu_ctx):
    """The full config (slope, spline with an elevation gradient, a Hann window, low + high pass, 2 modes) on D 32,
    T 5000: (a) op.apply of the raw signal is process_tod's output (the same kernels; the frozen-mode product is
    associated differently in float64, so within one float32 rounding, STEP_TOL of the row's maximum); (b) op.apply and
    op.apply_transpose equal the float64 reference with the same frozen U, n, per row within STEP_TOL times the 5
    float32-rounded steps times the row's largest magnitude along the reference's chain; (c) the device adjoint identity
    for three random pairs, |<F x, y> - <x, F^T y>| <= sum_rows eps (max|F x|_row |y_row|_1 + max|F^T y|_row |x_row|_1),
    eps = STEP_TOL times those 5 steps (the GEMM steps run in float64)."""
    import torch

    from maria_amd import tod_processing as tp
    from test_gpu_todproc import _tod

    D, T = 32, 5000
    tod, signal, t, el = _tod(D=D, T=T)
    raw = tp._signal(tod, torch.device(DEV))
    done, op = tp.preprocess_operator(tod, config=_copy(FULL), ctx=gpu_ctx, device=DEV)
    assert op.names == ["remove_slope", "remove_spline", "window", "filter", "remove_modes"] and op.shape == (D, T)
    plain = tp.process_tod(tod, config=_copy(FULL), ctx=gpu_ctx, device=DEV)
    assert torch.equal(plain.data["total"], done.data["total"]) and np.array_equal(plain.weight, done.weight)
    processed = done.data["total"].cpu().numpy()
    # (a)
    got = op.apply(raw.clone()).cpu().numpy()
    err = np.abs(got.astype(np.float64) - processed).max(axis=1) / np.abs(processed).max(axis=1)
    print(f"[filter-aware] op.apply(raw) vs process_tod: worst row {err.max():.2e} of its maximum; bit-equal "
          f"{(got == processed).mean():.6f}")
    assert err.max() <= STEP_TOL
    # (b)
    prod = op.product()
    assert prod["steps"] == op.names and prod["modes"].shape == (D, 2) and prod["row_norms"].shape == (D,)
    steps = ref.build(_copy(FULL), t, el, modes=(prod["modes"], prod["row_norms"]))
    rng = np.random.default_rng(7)
    eps = STEP_TOL * FULL_ROUNDED_STEPS
    x0 = raw.cpu().numpy()
    y0 = rng.normal(size=(D, T)).astype(np.float32)
    for name, v, transpose in (("apply", x0, False), ("apply_transpose", y0, True)):
        want, top = _chain(steps, v, transpose)
        buf = torch.as_tensor(v).to(DEV)
        out = (op.apply_transpose(buf) if transpose else op.apply(buf)).cpu().numpy().astype(np.float64)
        ratio = np.abs(out - want).max(axis=1) / top
        print(f"[filter-aware] op.{name} vs float64 reference: worst row {ratio.max():.2e} of the chain's maximum (bound {eps:.1e})")
        assert ratio.max() <= eps, ratio
    # (c)
    for i in range(3):
        x, y = (rng.normal(size=(D, T)).astype(np.float32) for _ in range(2))
        Fx = op.apply(torch.as_tensor(x).to(DEV)).cpu().numpy().astype(np.float64)
        Fty = op.apply_transpose(torch.as_tensor(y).to(DEV)).cpu().numpy().astype(np.float64)
        gap = abs(np.sum(Fx * y) - np.sum(x * Fty))
        bound = eps * np.sum(np.abs(Fx).max(axis=1) * np.abs(y).sum(axis=1) + np.abs(Fty).max(axis=1) * np.abs(x).sum(axis=1))
        print(f"[filter-aware] device adjoint identity, pair {i}: gap {gap:.3e}, bound {bound:.3e}")
        assert gap <= bound
    with pytest.raises(ValueError):
        op.apply(torch.zeros(D, T + 1, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        op.apply_transpose(torch.zeros(D, T, dtype=torch.float64, device=DEV))


def test_operator_of_a_long_cascade_and_a_bare_filter(gpu_ctx):
    """A cascade of more than 8 sections runs as consecutive launches, its transpose from the last to the first; and
    {"filter": {}} is the slope alone.  Both against the reference, as above."""
    import torch

    from maria_amd import tod_processing as tp
    from test_gpu_todproc import _tod

    tod, signal, t, el = _tod(D=9, T=3001)
    rng = np.random.default_rng(2)
    for config, rounded in (({"filter": {"f_lower": 0.1, "f_upper": 8.0, "order": 4}}, 2), ({"filter": {}}, 1)):
        done, op = tp.preprocess_operator(tod, config=_copy(config), ctx=gpu_ctx, device=DEV)
        steps = ref.build(_copy(config), t, el)
        for transpose in (False, True):
            v = rng.normal(size=(9, 3001)).astype(np.float32) + (0.0 if transpose else 20.0)
            want, top = _chain(steps, v, transpose)
            buf = torch.as_tensor(v).to(DEV)
            out = (op.apply_transpose(buf) if transpose else op.apply(buf)).cpu().numpy().astype(np.float64)
            ratio = np.abs(out - want).max(axis=1) / top
            print(f"[filter-aware] {config} transpose {transpose}: worst row {ratio.max():.2e}")
            assert ratio.max() <= STEP_TOL * rounded


# ---- 4, 7: the map against a dense solve ---------------------------------------------------------

MODES_CONFIG = {"filter": {"f_lower": 0.2}, "remove_modes": {"modes_to_remove": 1}}


def _pointing_matrix(probe, tod, shape):
    """P [D T, n] (scipy.sparse, float64): the columns mrx_map_project gives for unit maps."""
    import scipy.sparse

    from test_gpu_noise_filter import _project

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
    D, T = tod.dets.n, tod.coords.t.size
    return scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(D * T, n))


def _dense_system(P, steps, det_w, d):
    """A = (F P)^T W (F P), b = (F P)^T W F d in float64, F the reference operator column by column."""
    D, T = d.shape
    n = P.shape[1]
    FP = np.empty((D * T, n))
    Pc = P.tocsc()
    for j in range(n):
        FP[:, j] = ref.apply(steps, Pc[:, j].toarray().reshape(D, T)).ravel()
    Fd = ref.apply(steps, d.astype(np.float64)).ravel()
    w = np.repeat(det_w, T)
    WFP = FP * w[:, None]
    return FP.T @ WFP, WFP.T @ Fd


def _mapper_det_w(ctx, tod, config):
    """The mapper's "inverse_variance" weight: 1 / var of every pre-processed row (process_tod gives the same bits)."""
    from maria_amd import tod_processing as tp

    rows = tp.process_tod(tod, config=_copy(config), ctx=ctx, device=DEV).data["total"]
    return (1.0 / rows.double().var(dim=1)).cpu().numpy()


def _compare_with_dense(mapper, m, A, b, shape):
    """max |map - dense| over max |dense| on the solved pixels, each plane up to its hits-weighted mean."""
    n = int(np.prod(shape))
    solved = np.isfinite(m).ravel()
    assert solved.sum() >= 0.8 * n, solved.sum() / n
    dense = np.full(n, np.nan)
    dense[solved] = np.linalg.solve(A[np.ix_(solved, solved)], b[solved])
    dense, got = dense.reshape(shape), m.astype(np.float64)
    w = mapper.products["weight"][0, 0]
    err, scale = 0.0, 0.0
    for s in range(shape[0]):
        ok = np.isfinite(got[s, 0])
        r = got[s, 0][ok] - dense[s, 0][ok]
        r -= np.sum(w[ok] * r) / np.sum(w[ok])
        err = max(err, np.abs(r).max())
        scale = max(scale, np.abs(dense[s, 0][ok]).max())
    return err / scale


def _signal_for(P, shape, D, T, seed):
    """A smooth IQU sky through P plus a random walk per detector and one shared by all (what the removed mode picks up)."""
    from test_gpu_noise_filter import _smooth_iqu

    rng = np.random.default_rng(seed)
    d = (P @ _smooth_iqu(shape).ravel()).reshape(D, T) + 0.03 * np.cumsum(rng.normal(size=(D, T)), axis=1) / np.sqrt(T)
    d += np.outer(rng.uniform(0.9, 1.1, D), 0.5 * np.cumsum(rng.normal(size=T)) / np.sqrt(T))
    return d.astype(np.float32)


@pytest.mark.parametrize("bilinear", [False, True])
def test_map_matches_a_dense_solve(gpu_ctx, bilinear):
    """D 48, T 6000, a 12 x 16 IQU map, F = high pass at 0.2 Hz and one removed mode, tol 1e-8: the map equals the float64
    dense solve of (P^T F^T W F P) m = P^T F^T W F d on the solved pixels (P: mrx_map_project's columns for unit maps;
    F: the float64 reference with the mapper's own frozen U, n; W: the mapper's 1 / var weights), each plane up to its
    hits-weighted mean, within test_gpu_noise_filter's bound, 1e-6 of the dense map's maximum."""
    from maria_amd.mappers import MaximumLikelihoodMapper
    from test_gpu_noise_filter import _tods

    tod, az, el = _tods()
    D, T = tod.dets.n, tod.coords.t.size
    kw = dict(center=(az, el), width=16 * 0.05, height=12 * 0.05, resolution=0.05, stokes="IQU", frame="az/el", bilinear=bilinear,
              tol=1e-8, max_iter=400)
    probe = MaximumLikelihoodMapper([tod], **kw)
    shape = (3, 1, probe.n_eta, probe.n_xi)
    assert shape[2:] == (12, 16)
    P = _pointing_matrix(probe, tod, shape)
    tod.data = {"map": _signal_for(P, shape, D, T, seed=9)}
    mapper = MaximumLikelihoodMapper([tod], tod_preprocessing=_copy(MODES_CONFIG), filter_aware=True, **kw)
    m = mapper.run().data
    assert mapper.products["converged"] and mapper.products["filter_aware"] is True
    pre = mapper.products["preprocessing"]
    assert len(pre) == 1 and pre[0]["steps"] == ["filter", "remove_modes"] and pre[0]["modes"].shape == (D, 1)
    steps = ref.build(_copy(MODES_CONFIG), tod.coords.t, modes=(pre[0]["modes"], pre[0]["row_norms"]))
    A, b = _dense_system(P, steps, _mapper_det_w(gpu_ctx, tod, MODES_CONFIG), tod.data["map"])
    err = _compare_with_dense(mapper, m, A, b, shape)
    print(f"[filter-aware] dense solve (bilinear {bilinear}): max |map - dense| / max |dense| = {err:.2e}, "
          f"{mapper.products['n_iter']} iterations, |r|/|b| {mapper.products['residuals'][-1]:.1e}")
    assert err <= 1e-6, err


def test_two_tods_match_the_dense_solve_of_the_summed_system(gpu_ctx):
    """Two TODs of different length (6000 and 4000 samples, different scans' worth of data), each with its own frozen
    mode, in one mapper: the dense solve of the sum of the two systems, nearest pointing, at the bound above."""
    from maria_amd.mappers import MaximumLikelihoodMapper
    from test_gpu_noise_filter import _tods

    tod_a, az, el = _tods()
    tod_b, _, _ = _tods(T=4000, angles=(20.0, 65.0, 110.0, 155.0))
    kw = dict(center=(az, el), width=16 * 0.05, height=12 * 0.05, resolution=0.05, stokes="IQU", frame="az/el", tol=1e-8, max_iter=400)
    probe = MaximumLikelihoodMapper([tod_a, tod_b], **kw)
    shape = (3, 1, probe.n_eta, probe.n_xi)
    Ps = [_pointing_matrix(probe, tod, shape) for tod in (tod_a, tod_b)]
    for seed, (tod, P) in enumerate(zip((tod_a, tod_b), Ps)):
        tod.data = {"map": _signal_for(P, shape, tod.dets.n, tod.coords.t.size, seed=20 + seed)}
    mapper = MaximumLikelihoodMapper([tod_a, tod_b], tod_preprocessing=_copy(MODES_CONFIG), filter_aware=True, **kw)
    m = mapper.run().data
    assert mapper.products["converged"]
    pre = mapper.products["preprocessing"]
    assert len(pre) == 2 and not np.array_equal(pre[0]["modes"], pre[1]["modes"])
    A, b = 0.0, 0.0
    for tod, P, p in zip((tod_a, tod_b), Ps, pre):
        steps = ref.build(_copy(MODES_CONFIG), tod.coords.t, modes=(p["modes"], p["row_norms"]))
        Ai, bi = _dense_system(P, steps, _mapper_det_w(gpu_ctx, tod, MODES_CONFIG), tod.data["map"])
        A, b = A + Ai, b + bi
    err = _compare_with_dense(mapper, m, A, b, shape)
    print(f"[filter-aware] two TODs, dense solve: max |map - dense| / max |dense| = {err:.2e}, {mapper.products['n_iter']} iterations")
    assert err <= 1e-6, err


# ---- 5: what it is for --------------------------------------------------------------------------

@pytest.mark.parametrize("f_lower", [0.05, 0.2])
def test_extended_emission_survives_the_filter(gpu_ctx, f_lower):
    """24 detectors, 6000 samples at 50 Hz, a 16 x 16 nearest-pixel I map at 0.05 deg of a unit-peak Gaussian blob (sigma
    0.45 of the half width) under a common random walk 5 cumsum(N(0, 1)) / sqrt(T) with 10 % gain scatter and white noise
    of 0.01; F = slope removal, a Bessel order-1 high pass at ``f_lower`` and one removed mode.  The rms error of the
    filter-aware map over the observed pixels, hits-weighted mean removed, is at most a tenth of the plain
    MaximumLikelihoodMapper map's of the same TOD (float64 numpy gives 1/41 and 1/60), converged within 100 iterations
    (numpy: 14 and 18)."""
    from maria_amd.mappers import MaximumLikelihoodMapper
    from test_gpu_noise_filter import _project, _tods

    D, T = 24, 6000
    tod, az, el = _tods(D=D, T=T, angles=(0.0,))
    kw = dict(center=(az, el), width=16 * 0.05, resolution=0.05, stokes="I", frame="az/el", max_iter=100)
    config = {"remove_slope": {}, "filter": {"f_lower": f_lower, "order": 1}, "remove_modes": {"modes_to_remove": 1}}
    probe = MaximumLikelihoodMapper([tod], **kw)
    assert (probe.n_eta, probe.n_xi) == (16, 16)
    E, X = np.meshgrid(np.linspace(-1, 1, 16), np.linspace(-1, 1, 16), indexing="ij")
    truth = np.exp(-0.5 * (E**2 + X**2) / 0.45**2)
    rng = np.random.default_rng(int(1000 * f_lower))
    walk = 5.0 * np.cumsum(rng.normal(size=T)) / np.sqrt(T)
    d = (_project(probe, tod, truth.reshape(1, 1, 16, 16)).cpu().numpy().astype(np.float64)
         + np.outer(1.0 + 0.1 * rng.normal(size=D), walk) + 0.01 * rng.normal(size=(D, T)))
    tod.data = {"map": d.astype(np.float32)}

    def rms_error(mapper):
        m = mapper.run().data[0, 0].astype(np.float64)
        hits = mapper.products["weight"][0, 0]
        ok = np.isfinite(m)
        r = m[ok] - truth[ok]
        r -= np.sum(hits[ok] * r) / np.sum(hits[ok])
        return float(np.sqrt(np.mean(r**2))), int(ok.sum())

    plain = MaximumLikelihoodMapper([tod], tod_preprocessing=_copy(config), **kw)
    aware = MaximumLikelihoodMapper([tod], tod_preprocessing=_copy(config), filter_aware=True, **kw)
    e_plain, n_plain = rms_error(plain)
    e_aware, n_aware = rms_error(aware)
    print(f"[filter-aware] f_lower {f_lower} Hz: rms error plain {e_plain:.4f}, filter-aware {e_aware:.4f} (ratio 1/{e_plain / e_aware:.1f}) "
          f"over {n_aware} pixels, {aware.products['n_iter']} iterations, |r|/|b| {aware.products['residuals'][-1]:.1e}")
    assert n_aware == n_plain and n_aware > 0
    assert aware.products["converged"] and aware.products["n_iter"] <= 100
    assert e_aware <= 0.1 * e_plain, (e_aware, e_plain)


# ---- 6: identity and default --------------------------------------------------------------------

def _noisy_tod(seed=5):
    from test_gpu_noise_filter import _project, _smooth_iqu, _tods
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, az, el = _tods()
    kw = dict(center=(az, el), width=0.9, resolution=0.05, stokes="IQU", frame="az/el")
    probe = MaximumLikelihoodMapper([tod], **kw)
    shape = (3, 1, probe.n_eta, probe.n_xi)
    rng = np.random.default_rng(seed)
    tod.data = {"map": (_project(probe, tod, _smooth_iqu(shape)).cpu().numpy()
                        + 0.05 * rng.normal(size=(tod.dets.n, tod.coords.t.size))).astype(np.float32)}
    return tod, kw


def test_no_preprocessing_is_the_plain_map(gpu_ctx):
    """filter_aware=True with an empty tod_preprocessing: F = I and the map is the plain nearest-pixel solve within the CG
    tolerance, 1e-6 of the map's maximum, with the same NaN pattern."""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, kw = _noisy_tod()
    plain = MaximumLikelihoodMapper([tod], **kw)
    m_plain = plain.run().data
    aware = MaximumLikelihoodMapper([tod], filter_aware=True, tol=1e-9, **kw)
    m_aware = aware.run().data
    assert aware.products["converged"] and aware.products["preprocessing"] == [{"steps": []}]
    np.testing.assert_array_equal(np.isnan(m_plain), np.isnan(m_aware))
    ok = np.isfinite(m_plain)
    err = np.abs(m_aware[ok] - m_plain[ok]).max() / np.abs(m_plain[ok]).max()
    print(f"[filter-aware] F = I: max |filter-aware - plain| / max |plain| = {err:.2e} after {aware.products['n_iter']} iterations")
    assert err <= 1e-6, err


@pytest.mark.parametrize("bilinear", [False, True])
def test_the_default_is_the_path_it_was(gpu_ctx, bilinear):
    """filter_aware=False spelled out or left out: the same map bit for bit, no new products, with a pre-processing
    configured."""
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod, kw = _noisy_tod()
    kw = dict(kw, bilinear=bilinear, tod_preprocessing=_copy(MODES_CONFIG))
    left_out = MaximumLikelihoodMapper([tod], **kw)
    spelled = MaximumLikelihoodMapper([tod], filter_aware=False, **kw)
    a, b = left_out.run().data, spelled.run().data
    assert np.array_equal(a, b, equal_nan=True)
    expected = {"data", "weight", "blocks", "rhs", "residuals", "n_iter", "converged"}
    assert set(left_out.products) == expected and set(spelled.products) == expected
