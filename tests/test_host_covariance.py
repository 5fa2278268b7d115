"""The host side of maria_amd.covariance without a GPU: every Python-side refusal, ``finish_group``,
``leading_modes``, ``correlation_score``, ``judge`` and ``inject_uncorrelated`` against their numpy restatements, and the
two fixtures of the device tests judged by the float64 reference alone, with their margins."""

import os
import re

import covariance_ref as ref
import numpy as np
import pytest

from maria_amd import _lib, covariance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_BAND, T_FIX = 48, 4096
GROUPS = np.arange(2 * D_BAND) // D_BAND
INJECTED = [3, 17, 40, 55, 90]
CHUNK = 512  # TOD.cut's segments in the cut fixture


def one_over_f(rng, T, alpha=2.0, knee=64):
    """A unit-rms series of spectrum 1 / (1 + (f / f_knee)^alpha), f_knee = knee / T cycles a sample, less its mean."""
    f = np.fft.rfftfreq(T)
    shape = 1.0 / np.sqrt(1.0 + (f * T / knee) ** alpha)
    shape[0] = 0.0
    s = np.fft.irfft(shape * (rng.standard_normal(f.size) + 1j * rng.standard_normal(f.size)), T)
    return s / s.std()


def run_flags(rng, D, T, fraction, length=20):
    flags = np.zeros((D, T), np.uint8)
    for d in range(D):
        for s in rng.integers(0, T - length, int(fraction * T / length)):
            flags[d, s:s + length] = 1
    return flags


def modes_fixture():
    """Two bands of 48 detectors x 4096 samples.  Each band carries two 1/f modes: the first with loadings near 1 (12
    white levels strong), the second with loadings that run from -1 to 1 across the band (6 white levels), so that no
    rank-one common mode can take it.  White noise of level 1 (band 0) and 2 (band 1), offsets, 3 % of the samples flagged
    in runs of 20, and 1e30 under the flags.  Returns (x float32 with the 1e30, flags, sigma [D], clean x)."""
    rng = np.random.default_rng(21)
    D = 2 * D_BAND
    sigma = np.where(GROUPS == 0, 1.0, 2.0)
    x = np.zeros((D, T_FIX))
    for g in range(2):
        rows = np.flatnonzero(GROUPS == g)
        m1, m2 = one_over_f(rng, T_FIX), one_over_f(rng, T_FIX, knee=24)
        l1 = 1.0 + 0.1 * rng.standard_normal(D_BAND)
        l2 = np.linspace(-1.0, 1.0, D_BAND)
        x[rows] = sigma[rows, None] * (12.0 * l1[:, None] * m1[None] + 6.0 * l2[:, None] * m2[None])
    x += sigma[:, None] * rng.standard_normal((D, T_FIX)) + rng.uniform(-5, 5, (D, 1))
    flags = run_flags(rng, D, T_FIX, 0.03)
    clean = x.astype(np.float32)
    hostile = clean.copy()
    hostile[flags != 0] = np.float32(1e30)
    return hostile, flags, sigma, clean


def cut_fixture():
    """An atmosphere + noise TOD of the same size made on the host: per band a 1/f common mode seen with gains of
    1 +- 5 % and 5 white levels strong, a gradient across the band of 0.3 white levels at its edges, white noise whose level
    scatters by 10 % (and is 2.5 times higher in band 1).  Returns (clean float32 [96, 4096], the same with INJECTED made uncorrelated)."""
    rng = np.random.default_rng(33)
    D = 2 * D_BAND
    level = np.where(GROUPS == 0, 1.0, 2.5) * rng.uniform(0.9, 1.1, D)
    x = np.zeros((D, T_FIX))
    for g in range(2):
        rows = np.flatnonzero(GROUPS == g)
        gain = 1.0 + 0.05 * rng.standard_normal(D_BAND)
        slope = np.linspace(-1.0, 1.0, D_BAND)
        x[rows] = level[rows, None] * (5.0 * gain[:, None] * one_over_f(rng, T_FIX)[None] + 0.3 * slope[:, None] * one_over_f(rng, T_FIX)[None])
    x += level[:, None] * rng.standard_normal((D, T_FIX))
    clean = x.astype(np.float32)
    return clean, covariance.inject_uncorrelated(clean, INJECTED)


def residual_ceiling():
    """[96]: the most a detector's residual rms may exceed its white level by after remove_modes(2) on the modes fixture
    (derived in test_the_reference_removes_two_modes_where_one_and_the_common_mode_leave_the_second)."""
    l2 = np.linspace(-1.0, 1.0, D_BAND)
    rho2 = 0.03 * (12.0**2 / (6.0**2 * np.mean(l2**2))) / D_BAND
    return np.tile(1.03 * np.sqrt(1.0 + 36.0 * l2**2 * rho2), 2)


def rms_over_white(y, flags, sigma):
    keep = flags == 0
    e = np.where(keep, y.astype(np.float64), 0.0)
    n = keep.sum(axis=1)
    mu = e.sum(axis=1) / n
    return np.sqrt(np.where(keep, (y - mu[:, None]) ** 2, 0.0).sum(axis=1) / n) / sigma


def host_covariance(x, flags, groups, n_groups, min_hits=8):
    """``covariance.Covariance`` of host tensors from the float64 reference's G and n, through ``finish_group``."""
    import torch

    D = x.shape[0]
    mean, hits = ref.row_means(x, None, flags)
    z = ref.z_of(x, None, flags, mean)
    out, sigma, usable = [], torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.bool)
    for g in range(n_groups):
        rows = np.flatnonzero(groups == g)
        G, _ = ref.gram(z, rows)
        n = ref.counts(flags, D, x.shape[1], rows)
        cg = covariance.finish_group(torch.as_tensor(rows), torch.as_tensor(mean[rows]), torch.as_tensor(hits[rows]), torch.as_tensor(G),
                                     torch.as_tensor(n), min_hits)
        out.append(cg)
        sigma[cg.rows] = torch.where(cg.unusable, torch.zeros_like(cg.mean), torch.sqrt(torch.diagonal(cg.cov)))
        usable[cg.rows] = ~cg.unusable
    return covariance.Covariance(out, torch.as_tensor(groups.astype(np.int64)), torch.as_tensor(mean), sigma, usable, min_hits)


def test_the_block_constant_is_the_headers():
    text = open(os.path.join(ROOT, "include", "mrx.h")).read()
    (block,) = re.findall(r"#define MRX_GRAM_BLOCK (\d+)", text)
    B = int(block)
    assert _lib.GRAM_BLOCK == covariance.GRAM_BLOCK == B and B <= 1024 and B & (B - 1) == 0


def test_every_refusal_comes_before_a_device_call():
    """On host tensors every ValueError of ``gram`` and ``covariance`` is raised, the last of them "must be a device
    tensor": no device is touched (this machine may have none)."""
    import torch

    x = torch.zeros((4, 10), dtype=torch.float32)
    f = torch.zeros((4, 10), dtype=torch.uint8)
    bad = [
        (dict(x=x.double()), "float32"), (dict(x=x[:, ::2]), "unit stride"), (dict(x=torch.zeros((0, 3))), "D >= 1"),
        (dict(x=x, center=torch.zeros(4)), "center"), (dict(x=x, center=torch.zeros(3, dtype=torch.float64)), "center"),
        (dict(x=x, rows=np.zeros((2, 2), int)), "rows"), (dict(x=x, rows=np.array([], int)), "rows"), (dict(x=x, rows=np.array([0.5])), "rows"),
        (dict(x=x, rows=np.array([2**40])), "int32"), (dict(x=x, flags=f.float()), "flags"), (dict(x=x, flags=f[:, :9]), "flags"),
        (dict(x=x, model=x[:3]), "model"), (dict(x=x, model=x.double()), "model"), (dict(x=x), "device tensor"),
        (dict(x=x, rows=np.array([3, -1, 9]), center=torch.zeros(4, dtype=torch.float64), flags=f, model=x), "device tensor"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            covariance.gram(**kw)
    bad = [(dict(x=x, groups=np.zeros(3, int)), "groups"), (dict(x=x, groups=np.zeros(4)), "groups"), (dict(x=x, n_groups=0), "n_groups"),
           (dict(x=x, n_groups=17), "n_groups"), (dict(x=x, min_hits=-1), "min_hits"), (dict(x=x, flags=f[:3]), "flags"),
           (dict(x=x, model=x[:, :5]), "model"), (dict(x=x), "device tensor")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            covariance.covariance(**kw)
    with pytest.raises(ValueError, match="rows"):
        covariance.inject_uncorrelated(np.zeros((3, 5)), [3])
    with pytest.raises(ValueError, match="seed"):
        covariance.inject_uncorrelated(np.zeros((3, 5)), [1], seed=0.5)


def small_group(seed=2, R=9, T=400):
    import torch

    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, T)) + 2.0 * rng.standard_normal(T)[None] * rng.uniform(-1, 1, (R, 1))).astype(np.float32)
    flags = (rng.random((R, T)) < 0.2).astype(np.uint8)
    flags[4] = 1        # nothing kept
    x[6] = 3.0          # a constant row: G_ii == 0 about its mean
    flags[7, 5:] = 1    # fewer than min_hits kept
    mean, hits = ref.row_means(x, None, flags)
    G, _ = ref.gram(ref.z_of(x, None, flags, mean))
    n = ref.counts(flags, R, T)
    cg = covariance.finish_group(torch.arange(R), torch.as_tensor(mean), torch.as_tensor(hits), torch.as_tensor(G), torch.as_tensor(n), 8)
    return cg, G, n


def test_finish_group_modes_and_score_against_numpy():
    import torch

    cg, G, n = small_group()
    cov, corr, valid, unusable = ref.finish_group(G, n, 8)
    assert unusable.tolist() == [False] * 4 + [True, False, True, True, False]
    assert np.array_equal(cg.unusable.numpy(), unusable) and np.array_equal(cg.valid.numpy(), valid)
    assert np.array_equal(cg.cov.numpy(), cov) and np.array_equal(cg.corr.numpy(), corr)
    assert np.all(corr[unusable] == 0) and np.all(corr[:, unusable] == 0) and np.allclose(np.diag(corr)[~unusable], 1.0, rtol=0, atol=1e-15)
    for k in (1, 3, 6):
        w, U = covariance.leading_modes(cg, k)
        w_ref, U_ref = ref.leading_modes(corr, unusable, k)
        assert tuple(U.shape) == (9, k) and np.all(np.diff(w.numpy()) <= 0) and np.all(U.numpy()[unusable] == 0)
        np.testing.assert_allclose(w.numpy(), w_ref, rtol=1e-12)
        np.testing.assert_allclose(U.numpy(), U_ref, rtol=0, atol=1e-10)
        assert np.all(U.numpy().sum(axis=0) >= 0)  # the sign rule
        np.testing.assert_allclose(np.linalg.norm(U.numpy(), axis=0), 1.0, rtol=1e-12)
    for k in (0, 7, 1.5):
        with pytest.raises(ValueError, match="usable rows"):
            covariance.leading_modes(cg, k)
    # the sign rule on a matrix whose leading vector eigh may return with either sign
    flipped = cg._replace(corr=torch.as_tensor(np.where(np.outer(~unusable, ~unusable), 0.5 + 0.5 * np.eye(9), 0.0)))
    assert float(covariance.leading_modes(flipped, 1)[1].sum()) > 0
    score = covariance.correlation_score(cg).numpy()
    want = ref.correlation_score(corr, valid, unusable)
    assert np.array_equal(np.isnan(score), unusable) and np.array_equal(score[~unusable], want[~unusable])
    # an even and an odd number of partners, and a row whose pairs are all invalid
    lone = cg._replace(valid=cg.valid & ~torch.as_tensor(np.arange(9) == 0)[:, None] & ~torch.as_tensor(np.arange(9) == 0)[None, :])
    s2 = covariance.correlation_score(lone).numpy()
    assert np.isnan(s2[0]) and np.array_equal(s2[1:], ref.correlation_score(corr, lone.valid.numpy(), unusable)[1:], equal_nan=True)


def test_inject_uncorrelated_keeps_a_rows_statistics():
    import cuts_ref

    clean, dirty = cut_fixture()
    rest = np.setdiff1d(np.arange(clean.shape[0]), INJECTED)
    assert dirty.dtype == np.float32 and np.array_equal(dirty[rest], clean[rest]) and np.array_equal(dirty[INJECTED], clean[INJECTED][:, ::-1])
    a, b = (cuts_ref.summarize(cuts_ref.moments(v, None)) for v in (clean, dirty))
    for name in ("std", "sigma_diff", "kurtosis", "skew", "min", "max", "mean"):
        np.testing.assert_allclose(b[name], a[name], rtol=1e-9, atol=1e-12, err_msg=name)


def test_the_reference_removes_two_modes_where_one_and_the_common_mode_leave_the_second():
    """The modes fixture through the float64 reference alone.  remove_modes(2) leaves every detector at its white level:
    sqrt(1 - 2 / 48 - 1 / 4096) = 0.978 of it, which the estimate scatters about by 1 / sqrt(2 * 3900) = 1.1 %, so not below
    0.93; and not above ``ceiling``.  The ceiling is what the flags cost.  A template is the projection S / W of the rows
    that keep the sample onto one loading; where a row is flagged the loadings are no longer orthogonal on the rows that
    are left, and the strong first mode leaks into the second template by -U_d2 U_d1 a_1(t) / W for each flagged row d.
    With a fraction f = 0.03 flagged, D = 48 rows and mean U^2 = 1 / D, that is a share rho^2 = f lambda_1 / (D lambda_2)
    of the second template's variance, lambda_1 / lambda_2 = 12^2 / (6^2 mean(l2^2)) = 11.5 by the fixture's design; a
    detector of loading l2 carries 6 l2 white levels of that template, so its residual is within
    sqrt(1 + 36 l2^2 rho^2), 1.12 at the band's edge, times 1.03 for the scatter.  Without flags the figure is 0.94 .. 1.01.
    remove_modes(1) and the common mode leave the second mode, 6 white levels times its loading: the detectors of the band's
    outer thirds (|loading| > 1 / 3) stay above 2 white levels."""
    import regress_ref as rr

    x, flags, sigma, _ = modes_fixture()
    assert 0.02 < (flags != 0).mean() < 0.04
    y2, B, a, eig, U = ref.remove_modes(x, flags, GROUPS, 2, ref.gram_of_data(x, flags), 2)
    r2 = rms_over_white(y2, flags, sigma)
    y1 = ref.remove_modes(x, flags, GROUPS, 2, ref.gram_of_data(x, flags), 1)[0]
    r1 = rms_over_white(y1, flags, sigma)
    _, ac, _, ok, Bc = rr.fit_common_mode(x, groups=GROUPS, n_groups=2, flags=flags)
    rc = rms_over_white(rr.apply(x, Bc, ac, groups=GROUPS, sign=-1), flags, sigma)
    outer = np.abs(np.linspace(-1, 1, D_BAND)) > 1 / 3
    outer = np.concatenate([outer, outer])
    print(f"reference: residual rms / white after remove_modes(2) {r2.min():.4f} .. {r2.max():.4f}; outer thirds after remove_modes(1) "
          f">= {r1[outer].min():.3f}, after remove_common_mode >= {rc[outer].min():.3f}; eigenvalues {eig.round(2).tolist()}")
    assert ok.all() and np.all(eig[:, 1] > 3.0) and np.all((r2 >= 0.93) & (r2 <= residual_ceiling()))
    assert np.all(r1[outer] > 2.0) and np.all(rc[outer] > 2.0)
    # the second loading changes sign across the band, the first does not
    for g in range(2):
        u1, u2 = U[GROUPS == g, 0], U[GROUPS == g, 1]
        assert np.all(u1 > 0) and (u2 > 0).sum() >= 16 and (u2 < 0).sum() >= 16


def test_the_reference_cuts_exactly_the_injected_rows_and_the_statistics_cut_none_of_them():
    """The cut fixture through the float64 reference alone: ``judge`` takes exactly the injected rows, with room on both
    sides of the threshold, and the rules of TOD.cut, which look at one row at a time, take none of them."""
    from test_host_cuts import reference_verdict

    from maria_amd import cuts

    clean, dirty = cut_fixture()
    cov = host_covariance(dirty, None, GROUPS, 2)
    verdict = {k: v.numpy() for k, v in covariance.judge(cov).items()}
    score = verdict["score"]
    want_score = np.full(96, np.nan)
    for g, cg in enumerate(cov.groups):
        want_score[GROUPS == g] = ref.correlation_score(cg.corr.numpy(), cg.valid.numpy(), cg.unusable.numpy())
    cut, median, threshold = ref.judge(want_score, GROUPS, np.ones(96, bool))
    assert np.array_equal(score, want_score) and np.array_equal(verdict["cut"], cut) and np.array_equal(verdict["threshold"], threshold)
    live = np.setdiff1d(np.arange(96), INJECTED)
    room = [(score[live][GROUPS[live] == g].min(), score[[d for d in INJECTED if GROUPS[d] == g]].max(), median[g], threshold[g]) for g in range(2)]
    print("per band (lowest live score, highest injected score, median, threshold): " + ", ".join(str(tuple(round(float(v), 4) for v in r)) for r in room))
    assert np.flatnonzero(cut).tolist() == INJECTED and not verdict["unusable"].any() and not verdict["below"].any()
    for lo_live, hi_injected, med, thr in room:  # the live rows use at most 4 of the 5 scales to the threshold, the injected lie 50 beyond the median
        assert med - lo_live <= 0.8 * (med - thr) and med - hi_injected >= 10.0 * (med - thr)
    assert np.flatnonzero(covariance.judge(cov, min_correlation=0.5)["cut"].numpy()).tolist() == INJECTED
    _, cut_by_stats, _, _ = reference_verdict(dirty, cuts.chunk_bounds(T_FIX, CHUNK), None, GROUPS)
    print(f"TOD.cut's rules on the same data cut {cut_by_stats}")
    assert not set(cut_by_stats) & set(INJECTED)
    # on the clean data nothing is cut
    assert not covariance.judge(host_covariance(clean, None, GROUPS, 2))["cut"].any()
