"""The host side of the frozen subscan projector (maria_amd.subscans.freeze / project / Projector and
MaximumLikelihoodMapper(subscan_filter=...)) without a GPU: ``freeze`` on CPU torch against ``regress.solve``
and a longdouble solve, the operator's identities on the dense float64 reference of tests/subscan_project_ref.py, and every
Python-side refusal."""

import numpy as np
import pytest
import subscan_project_ref as pref
import subscans_ref as ref
import torch

from maria_amd import regress, subscans


def systems(seed=0):
    """(N [D, S, K, K], r [D, S, K], hits [D, S]) per K = 1 .. 8: 6 rows of Gaussian data in segments of 0 .. 600 samples,
    30 % flagged, one segment wholly flagged, one with fewer kept samples than min_hits."""
    rng = np.random.default_rng(seed)
    bounds = np.concatenate([[3], 3 + np.cumsum([150, 0, 600, 33, 257, 9, 300, 64])]).astype(np.int32)
    D, T = 6, int(bounds[-1]) + 5
    x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
    flags = (rng.random((D, T)) < 0.3).astype(np.uint8)
    flags[2, bounds[2]:bounds[3]] = 1
    flags[4, bounds[5]:bounds[6] - 4] = 1
    for K in range(1, 9):
        N, r, hits, _, _ = ref.normal_equations(x, bounds, K, flags=flags)
        yield K, N, r, hits


def _rel(a, want):
    """max over the systems of max_i |a_i - want_i| / max_i |want_i|."""
    top = np.abs(want).max(axis=-1)
    return float((np.abs(a - want).max(axis=-1) / np.where(top > 0, top, 1.0)).max())


def test_freeze_agrees_with_solve():
    """``ok`` is ``regress.solve``'s verdict exactly, A is zero where a pair is not ok, and the ordered product A r agrees
    with ``solve``'s a on the same systems (K = 1 .. 8, segments of 9 .. 600 samples, 30 % flagged).

    Both are first measured against a longdouble Cholesky solve of the same float64 N and r, as
    max_i |a_i - a_ld_i| / max_i |a_ld_i| over the systems: ``solve`` 8.6e-15, A r 1.13e-14 (both at K = 8; 3.2e-16 and
    5.6e-16 at K = 4).  The bound on |A r - a_solve| / max |a_solve| is 4 x the larger, 4.5e-14; measured 4.0e-15."""
    bound = 4 * 1.13e-14
    worst = {"solve": 0.0, "A r": 0.0, "gap": 0.0}
    for K, N, r, hits in systems():
        D, S = hits.shape
        tN, tr, th = torch.as_tensor(N), torch.as_tensor(r), torch.as_tensor(hits)
        a, ok = regress.solve(tN.view(D * S, K, K), tr.view(D * S, K), th.view(D * S))
        A, ok_f = subscans.freeze(tN, th)
        assert A.dtype == torch.float64 and tuple(A.shape) == (D, S, K, K) and ok_f.dtype == torch.uint8 and tuple(ok_f.shape) == (D, S)
        assert torch.equal(ok_f.bool(), ok.view(D, S))
        A, ok, a = A.numpy(), ok.view(D, S).numpy(), a.view(D, S, K).numpy()
        assert not ok[2, 2] and not ok[4, 5] and not ok[:, 1].any() and ok.sum() >= 30
        assert not A[~ok].any() and np.all(np.diagonal(A[ok], axis1=1, axis2=2) > 0)
        ar = pref.ordered_product(A, r)
        a_ld = pref.solve_longdouble(N, r, ok)
        e_solve, e_ar, gap = _rel(a[ok], a_ld[ok]), _rel(ar[ok], a_ld[ok]), _rel(ar[ok], a[ok])
        print(f"K {K}: solve vs longdouble {e_solve:.2e}, A r vs longdouble {e_ar:.2e}, A r vs solve {gap:.2e}")
        worst = {"solve": max(worst["solve"], e_solve), "A r": max(worst["A r"], e_ar), "gap": max(worst["gap"], gap)}
        # the reference's freeze is the same steps: its verdict is the same and its A agrees to the solves' accuracy
        A_ref, ok_ref = pref.freeze(N, hits)
        assert np.array_equal(ok_ref != 0, ok) and _rel(pref.ordered_product(A_ref, r)[ok], a_ld[ok]) <= bound
    print(f"worst: {worst}; bound {bound:.2e}")
    assert worst["gap"] <= bound


def test_frozen_inverse_is_symmetric_bit_for_bit():
    for K, N, _, hits in systems(seed=1):
        A, _ = subscans.freeze(torch.as_tensor(N), torch.as_tensor(hits))
        A = A.numpy()
        assert np.array_equal(A.view(np.uint64), np.ascontiguousarray(A.transpose(0, 1, 3, 2)).view(np.uint64)), K
    # min_hits and rcond reach the verdict
    K, N, _, hits = next(s for s in systems() if s[0] == 3)
    _, ok = subscans.freeze(torch.as_tensor(N), torch.as_tensor(hits), min_hits=200)
    assert np.array_equal(ok.numpy() != 0, hits >= 200)
    _, ok = subscans.freeze(torch.as_tensor(N), torch.as_tensor(hits), rcond=0.999)
    assert 0 < ok.sum() < (hits >= 8).sum()  # P_0, P_1, P_2 are all but orthogonal on a few of these masks only


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_identities_on_the_dense_reference(K):
    """On segments of L = 33, 64 and 257 samples (L >= 4 K) with 30 % flagged, in float64: F'^2 = F', F' T = 0,
    F' F = F' for the filter F of a smaller mask (the flags grew since), and F'^t W F' = W F' for W = w M.

    Every entry of these matrices is a sum of at most 257 products of entries that are O(K) (|P_i| <= 1, the scaled
    inverse's entries below its condition number, < 1e3 here): 257 * 2^-53 * 1e3 = 3e-11 a product, so 1e-10 bounds the
    difference of two such matrices with room; measured <= 2e-13."""
    rng = np.random.default_rng(K)
    worst = 0.0
    for L in (33, 64, 257):
        early = rng.random(L) >= 0.15         # what was kept when F was applied
        keep = early & (rng.random(L) >= 0.15)  # the final mask: more is flagged
        A, ok = pref.segment_inverse(L, K, keep)
        A0, ok0 = pref.segment_inverse(L, K, early)
        assert ok and ok0
        Fp, F = pref.dense(L, K, keep, A), pref.dense(L, K, early, A0)
        Tm = ref.basis(L, K).T
        W = np.diag(2.5 * keep)
        gaps = [np.abs(Fp @ Fp - Fp).max(), np.abs(Fp @ Tm).max(), np.abs(Fp @ F - Fp).max(), np.abs(Fp.T @ W @ Fp - W @ Fp).max(),
                np.abs(pref.dense(L, K, keep, A, transpose=True) - Fp.T).max()]
        worst = max(worst, *gaps)
    print(f"K {K}: largest gap {worst:.2e}")
    assert worst <= 1e-10


def test_reference_project_is_the_dense_operator():
    """``pref.project`` and ``pref.Frozen`` restate the dense F and F^t; a pair that cannot be fitted is the identity."""
    rng = np.random.default_rng(5)
    bounds = np.array([2, 40, 40, 45, 140], np.int32)
    D, T, K = 3, 145, 3
    x = rng.standard_normal((D, T))
    flags = (rng.random((D, T)) < 0.2).astype(np.uint8)
    frozen = pref.Frozen(D, T, bounds, K, flags, unfitted=[(d, 2) for d in range(D)])
    for transpose in (False, True):
        y, ok = pref.project(x, bounds, K, flags=flags, transpose=transpose)
        assert ok[:, [0, 3]].all() and not ok[:, [1, 2]].any()
        assert np.array_equal(y[:, :2], x[:, :2]) and np.array_equal(y[:, 40:45], x[:, 40:45]) and np.array_equal(y[:, 140:], x[:, 140:])
        for d in range(D):
            keep = flags[d, 45:140] == 0
            A, _ = pref.segment_inverse(95, K, keep)
            np.testing.assert_allclose(y[d, 45:140], pref.dense(95, K, keep, A, transpose) @ x[d, 45:140], rtol=0, atol=1e-12)
        np.testing.assert_allclose(frozen.apply_transpose(x) if transpose else frozen.apply(x), y, rtol=0, atol=1e-12)


# ---- refusals ------------------------------------------------------------------------------------

def _operands(D=3, T=50, S=2, K=2):
    x = torch.zeros((D, T), dtype=torch.float32)
    A = torch.zeros((D, S, K, K), dtype=torch.float64)
    ok = torch.ones((D, S), dtype=torch.uint8)
    return x, np.array([0, 20, T], np.int32), A, ok


def test_project_refusals_need_no_device():
    x, bounds, A, ok = _operands()
    D, T = x.shape
    flags = torch.zeros((D, T), dtype=torch.uint8)
    bad = [
        dict(x=x.double()), dict(x=x[0]), dict(x=x.t()), dict(x=torch.zeros((0, T))),
        dict(bounds=np.array([0, 30, 20])), dict(bounds=np.array([0.0, 20.0])), dict(bounds=np.array([5])), dict(bounds=np.array([[0, 5]])),
        dict(A=A.float()), dict(A=A[:, :1]), dict(A=A[..., :1]), dict(A=A.numpy()), dict(A=torch.zeros((D, 2, 9, 9), dtype=torch.float64)),
        dict(ok=ok.to(torch.int32)), dict(ok=ok[:, :1]), dict(ok=ok.numpy()),
        dict(flags=flags.bool()), dict(flags=flags[:, :-1]), dict(flags=flags.numpy()),
        dict(transpose=1), dict(transpose=None),
    ]
    for kw in bad:
        args = dict(x=x, bounds=bounds, A=A, ok=ok, flags=flags, transpose=False)
        args.update(kw)
        with pytest.raises(ValueError) as err:
            subscans.project(args.pop("x"), args.pop("bounds"), args.pop("A"), args.pop("ok"), **args)
        assert "device tensor" not in str(err.value) or "on x's device" in str(err.value), kw
    with pytest.raises(ValueError, match="x must be a device tensor"):  # the last refusal
        subscans.project(x, bounds, A, ok, flags=flags)
    with pytest.raises(ValueError, match="x must be a device tensor"):
        subscans.project(x, bounds, A, ok, transpose=True, coefficients=True)


def test_freeze_refusals():
    K, N, _, hits = next(s for s in systems() if s[0] == 2)
    tN, th = torch.as_tensor(N), torch.as_tensor(hits)
    for args, kw in [((N, th), {}), ((tN.float(), th), {}), ((tN[0], th), {}), ((tN[..., :1], th), {}), ((tN, hits), {}), ((tN, th[:, :2]), {}),
                     ((tN, th.double()), {}), ((tN, th), dict(min_hits=-1)), ((tN, th), dict(min_hits=2.5)), ((tN, th), dict(rcond=1.0)),
                     ((tN, th), dict(rcond=-1e-3)), ((torch.zeros((2, 2, 9, 9), dtype=torch.float64), th[:2, :2]), {})]:
        with pytest.raises(ValueError):
            subscans.freeze(*args, **kw)


def _scan_tod(D=4, flags=None, recorded=None):
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates, Plan
    from test_host_subscans import SCAN

    plan = Plan.back_and_forth(start_time=1.7e9, scan_center=(120.0, 55.0), **SCAN)
    dets = Detectors(np.zeros((D, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int))
    meta = {} if recorded is None else {"subscans": recorded}
    return TOD({"signal": np.zeros((D, plan.time.size), np.float32)}, dets, Coordinates(plan.time, plan.phi, plan.theta), units="K_RJ",
               metadata=meta, flags=flags)


def test_mapper_keyword_refusals_need_no_device():
    from maria_amd.mappers import MaximumLikelihoodMapper

    record = {"order": 2, "bounds": np.array([0, 1000, 3000], np.int32), "turn_frac": 0.9, "min_hits": 8, "rcond": 1e-10,
              "coefficients": np.zeros((4, 2, 3)), "failed_segments": np.zeros((0, 2), np.int64)}
    plain, filtered = _scan_tod(), _scan_tod(recorded=record)
    kw = dict(center=(120.0, 55.0), width=1.0, resolution=0.1, stokes="I", frame="az/el")
    good = {"order": 3, "bounds": None, "turn_frac": 0.9, "min_hits": 8, "rcond": 1e-10}
    refused = [
        ([plain], dict(subscan_filter=good)),                                          # needs filter_aware=True
        ([plain], dict(subscan_filter=good, filter_aware=False)),
        ([filtered], dict(subscan_filter="recorded")),
        ([plain], dict(subscan_filter=good, filter_aware=True, noise_model="fit")),      # stays refused with filter_aware
        ([plain], dict(subscan_filter=good, filter_aware=True, noise_model="fit", noise_modes=1)),
        ([plain], dict(subscan_filter="recorded", filter_aware=True)),                   # no metadata["subscans"]
        ([filtered, plain], dict(subscan_filter="recorded", filter_aware=True)),
        ([plain], dict(subscan_filter="fitted", filter_aware=True)),
        ([plain], dict(subscan_filter=3, filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, degree=3), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, order=8), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, order=-1), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, order=1.5), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, bounds=[0, 200, 100]), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, bounds=[0.0, 200.0]), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, turn_frac=1.5), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, min_hits=-1), filter_aware=True)),
        ([plain], dict(subscan_filter=dict(good, rcond=1.0), filter_aware=True)),
        ([plain, filtered], dict(subscan_filter=[good], filter_aware=True)),            # one entry per TOD
        ([plain], dict(subscan_filter=[good, good], filter_aware=True)),
    ]
    for tods, extra in refused:
        with pytest.raises(ValueError):
            MaximumLikelihoodMapper(tods, **kw, **extra)
    # what is accepted, resolved on the host
    assert MaximumLikelihoodMapper([plain], **kw).subscan_filter is None
    assert MaximumLikelihoodMapper([plain], filter_aware=True, subscan_filter=None, **kw).subscan_filter is None
    found, _ = subscans.find_subscans(plain.coords._baz)
    m = MaximumLikelihoodMapper([plain, filtered], filter_aware=True, subscan_filter=[{"order": 1}, "recorded"], **kw)
    assert [s["order"] for s in m.subscan_filter] == [1, 2] and m.subscan_filter[0]["bounds"].tolist() == found.tolist()
    assert m.subscan_filter[1]["bounds"].tolist() == [0, 1000, 3000] and m.subscan_filter[0]["min_hits"] == 8
    m = MaximumLikelihoodMapper([filtered], filter_aware=True, subscan_filter="recorded", **kw)
    assert m.subscan_filter[0] == {"order": 2, "bounds": m.subscan_filter[0]["bounds"], "min_hits": 8, "rcond": 1e-10}
    m = MaximumLikelihoodMapper([plain], filter_aware=True, subscan_filter={"bounds": np.arange(0, 3001, 300)}, **kw)
    assert m.subscan_filter[0]["order"] == 3 and m.subscan_filter[0]["bounds"].dtype == np.int32 and len(m.subscan_filter[0]["bounds"]) == 11


# ---- the cases of the device's dense comparison (tests/test_gpu_subscan_project.py) and their bound ------------------

def dense_case(K, transpose):
    """(x float32, flags, bounds, y64, bound): 3 rows of 3 segments of 257 samples (L >= 4 K), 30 % flagged, and the float64
    reference's F x (or F^t x).  With p64 = x - y64 the polynomial taken out, the device's y = x - (float)p differs from y64
    by at most 2^-24 |p64| (p rounded to float32) + 2^-24 |y64| (the float32 difference, rounded) per sample, plus the
    float64 error of p itself: 4 x the largest |y64 - y_longdouble| of the case, the reference's own float64 error
    measured against its longdouble rebuild (7e-15 .. 3e-14 here, beside float32 terms of 1e-7 and more)."""
    rng = np.random.default_rng(100 * K + transpose)
    bounds = np.array([1, 258, 515, 772], np.int32)
    x = (rng.standard_normal((3, 774)) * 3 + 5).astype(np.float32)
    flags = (rng.random((3, 774)) < 0.3).astype(np.uint8)
    y64, ok = pref.project(x, bounds, K, flags=flags, transpose=bool(transpose))
    y_ld, _ = pref.project(x, bounds, K, flags=flags, transpose=bool(transpose), dtype=np.longdouble)
    assert ok.all()
    f64_term = 4.0 * float(np.abs(y64 - y_ld.astype(np.float64)).max())
    p64 = x.astype(np.float64) - y64
    return x, flags, bounds, y64, 2.0**-24 * (np.abs(p64) + np.abs(y64)) + f64_term, f64_term


@pytest.mark.parametrize("K", range(1, 9))
def test_the_dense_cases_reference_stays_inside_its_own_bound(K):
    """The reference's polynomial put through the device's two float32 roundings stays inside the bound the device is
    held to: the cases are well conditioned enough for the bound to be about the device."""
    for transpose in (0, 1):
        x, flags, bounds, y64, bound, f64_term = dense_case(K, transpose)
        p32 = (x.astype(np.float64) - y64).astype(np.float32)
        y32 = np.where((flags == 0) | (transpose == 0), x - p32, x).astype(np.float32)
        ratio = float((np.abs(y32.astype(np.float64) - y64) / bound).max())
        print(f"K {K} transpose {transpose}: float64 term {f64_term:.2e}, reference through float32 / bound {ratio:.3f}")
        assert f64_term <= 1e-10 and ratio <= 1.0
