"""maria_amd.lines on the host: the numpy reference of tests/lines_ref.py against numpy.linalg.lstsq, every
Python refusal, the line finder on synthetic spectra, the phase-slope refinement, the science fixture's margin, and the
size of the mistakes that the bounds of tests/test_gpu_lines.py must see, on that file's own inputs (which live here)."""

import math

import lines_ref as ref
import numpy as np
import pytest

from maria_amd import lines

ROWS = [1, 3, 65]
TIMES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097]
LENGTHS = [0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1024, 1025, 2049]
COMBOS = [(n_poly, L) for n_poly in range(3) for L in range(1, 4)]
HALF_ULP = 2.0**-53
# the carriers' allowance: 2 ulp for the device's float64 sinpi and cospi (the figure the HIP math documentation gives for
# both) and 1 ulp for the reference, an ulp taken at 1, the carriers' largest magnitude (DESIGN 3.37 has the measurement)
EPS_CARRIER = 3 * 2.0**-52


# ---- the inputs of the device tests ----

def make_bounds(T, seed):
    """[S + 1] int32: the LENGTHS in a random order from sample min(2, T // 3) on, as many as fit before the last
    min(3, T // 3) samples: some samples in no segment at both ends (from T = 3)."""
    rng = np.random.default_rng(seed)
    b = [min(2, T // 3)]
    for n in rng.permutation(LENGTHS):
        if b[-1] + n <= T - min(3, T // 3):
            b.append(b[-1] + int(n))
    if len(b) == 1:
        b.append(b[0])
    return np.array(b, np.int32)


def generic_nu(D, L, seed):
    """[D, L] frequencies in cycles a sample: generic (no short period), different in every row, in three separate bands."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.03 + 0.15 * l, 0.15 + 0.15 * l, D) for l in range(L)], axis=1)


def rows(D, T, seed, exact, flagged=0.3):
    """(x, model, flags): small integers (exact sums) or Gaussian; flags random at ``flagged``, values 1 and 2."""
    rng = np.random.default_rng(seed)
    if exact:
        x = rng.integers(-64, 65, (D, T)).astype(np.float32)
        model = rng.integers(-16, 17, (D, T)).astype(np.float32)
    else:
        x = (rng.standard_normal((D, T)) * 3 + 5).astype(np.float32)
        model = rng.standard_normal((D, T)).astype(np.float32)
    flags = ((rng.random((D, T)) < flagged) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    return x, model, flags


def quarter_nu(D, L):
    """[D, L] of 1/4 and 1/2 cycle a sample, alternating: every carrier is exactly 0 or +-1."""
    return np.array([[0.25, 0.5][(d + l) % 2] for d in range(D) for l in range(L)]).reshape(D, L)


def sum_bounds(bounds, aN, ar, dN, dr):
    """The acceptance of a device sum against the reference's fsum: (n + 1) 2^-53 sum|terms| for the summation order and
    fsum's own rounding, and EPS_CARRIER sum|d term / d carrier| for the carriers."""
    n = np.maximum(np.diff(np.asarray(bounds, np.int64)), 0).astype(np.float64)
    return (n[None, :, None, None] + 1) * HALF_ULP * aN + EPS_CARRIER * dN, (n[None, :, None] + 1) * HALF_ULP * ar + EPS_CARRIER * dr


def test_the_bounds_of_the_cases_hold_every_length():
    used = set()
    for K in range(1, 9):
        for T in TIMES:
            b = make_bounds(T, 10 * K + T)
            assert len(b) >= 2 and b[0] >= 0 and b[-1] <= T and (T < 3 or (b[0] > 0 and b[-1] < T))
            used |= set(np.diff(b).tolist())
    assert used == set(LENGTHS)


# ---- the reference ----

def test_sincospi_is_exact_at_the_quarter_cycles_and_close_elsewhere():
    x = np.arange(-8, 9) * 0.5
    s, c = ref.sincospi(x)
    assert s.tolist() == [0.0, 1.0, 0.0, -1.0] * 4 + [0.0] and c.tolist() == [1.0, 0.0, -1.0, 0.0] * 4 + [1.0]
    assert np.cos(np.pi * 0.5) != 0.0  # numpy's is not
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, 20000)
    s, c = ref.sincospi(x)
    assert np.abs(s - np.sin(np.pi * x)).max() < 4e-16 and np.abs(c - np.cos(np.pi * x)).max() < 4e-16
    assert np.abs(s * s + c * c - 1).max() < 5e-16
    nan = ref.sincospi(np.array([np.nan, np.inf]))
    assert np.isnan(nan[0]).all() and np.isnan(nan[1]).all()


def test_the_phase_counts_from_the_start_of_the_row():
    nu = np.array([0.1234567, 0.25])
    lo, hi = 1000, 1010
    B = ref.basis(lo, hi, nu, 2)
    t = np.arange(lo, hi)
    assert np.array_equal(B[0], np.ones(10)) and B[1, 0] == -1.0 and B[1, -1] == 1.0
    assert np.abs(B[2] - np.cos(2 * np.pi * nu[0] * t)).max() < 1e-12 and np.abs(B[3] - np.sin(2 * np.pi * nu[0] * t)).max() < 1e-12
    assert B[4].tolist() == [1.0, 0.0, -1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 1.0, 0.0] and B[5].tolist() == [0.0, 1.0, 0.0, -1.0] * 2 + [0.0, 1.0]


@pytest.mark.parametrize("n_poly,L", COMBOS)
def test_reference_fit_against_lstsq(n_poly, L):
    D, T = 3, 700
    x, model, flags = rows(D, T, 7 + n_poly + 3 * L, exact=False, flagged=0.2)
    nu = generic_nu(D, L, 5)
    bounds = np.array([3, 260, 260, 690], np.int32)
    a, ok = ref.fit(x, bounds, nu, n_poly, flags=flags, model=model)
    assert ok[:, [0, 2]].all() and not ok[:, 1].any() and not a[:, 1].any()
    for d in range(D):
        for s, (lo, hi) in enumerate(ref.segments(bounds, T)):
            if hi <= lo:
                continue
            keep = flags[d, lo:hi] == 0
            A = ref.basis(lo, hi, nu[d], n_poly)[:, keep].T
            y = x[d, lo:hi][keep].astype(np.float64) - model[d, lo:hi][keep].astype(np.float64)
            want = np.linalg.lstsq(A, y, rcond=None)[0]
            assert np.abs(a[d, s] - want).max() <= 1e-10 * np.abs(want).max(), (d, s)
    fast = ref.fit_fast(x, bounds, nu, n_poly, flags=flags, model=model)
    assert np.abs(fast[0] - a).max() <= 1e-11 * np.abs(a).max() and np.array_equal(fast[1], ok)


def test_reference_application_and_amplitude_phase():
    D, T, n_poly = 2, 300, 1
    nu = generic_nu(D, 2, 1)
    bounds = np.array([5, 100, 290], np.int32)
    rng = np.random.default_rng(2)
    amp, phi = rng.uniform(0.5, 2, (D, 2, 2)), rng.uniform(-3, 3, (D, 2, 2))
    a = np.zeros((D, 2, 5))
    a[:, :, 0] = 99.0  # a baseline coefficient: never applied
    a[:, :, 1::2], a[:, :, 2::2] = amp * np.cos(phi), -amp * np.sin(phi)
    got_amp, got_phi = lines.amplitude_phase(a, n_poly)
    assert np.allclose(got_amp, amp, rtol=1e-14) and np.allclose(got_phi, phi, rtol=1e-13)
    assert np.array_equal(np.stack(ref.amplitude_phase(a, n_poly)), np.stack([got_amp, got_phi]))
    y = ref.apply(np.zeros((D, T), np.float32), bounds, nu, a, n_poly, sign=+1)
    t = np.arange(T)
    for d in range(D):
        for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            want = sum(amp[d, s, l] * np.cos(2 * np.pi * nu[d, l] * t[lo:hi] + phi[d, s, l]) for l in range(2))
            assert np.abs(y[d, lo:hi] - want).max() < 1e-6
    assert not y[:, :5].any() and not y[:, 290:].any()


# ---- refusals ----

def test_python_refusals():
    import torch

    x = torch.zeros((4, 100), dtype=torch.float32)
    bounds = np.array([0, 50, 100], np.int32)
    nu = np.full((4, 2), 0.1)
    a = torch.zeros((4, 2, 5), dtype=torch.float64)
    bad_nu = [np.full((4, 4), 0.1), np.full((3, 2), 0.1), np.zeros((4, 0)), [0.0], [0.6], [-0.1], [np.nan], [np.inf], np.full((4, 2, 1), 0.1)]
    for v in bad_nu:
        with pytest.raises(ValueError, match="nu"):
            lines.normal_equations(x, bounds, v)
        with pytest.raises(ValueError, match="nu"):
            lines.refine(x, bounds, v)
    for n_poly in (-1, 3, 1.5, True):
        with pytest.raises(ValueError, match="n_poly"):
            lines.normal_equations(x, bounds, nu, n_poly=n_poly)
        with pytest.raises(ValueError, match="n_poly"):
            lines.apply(x, bounds, nu, a, n_poly)
    for b in ([0], [5, 3], np.array([0.0, 10.0]), [[0, 1]]):
        with pytest.raises(ValueError, match="bounds"):
            lines.normal_equations(x, b, nu)
        with pytest.raises(ValueError, match="bounds"):
            lines.apply(x, b, nu, a, 1)
    for v in (x.double(), x[0], torch.zeros((4, 100, 1)), x.t(), np.zeros((4, 100), np.float32)):
        with pytest.raises(ValueError, match="x must|x of shape"):
            lines.normal_equations(v, bounds, nu)
    with pytest.raises(ValueError, match="flags"):
        lines.normal_equations(x, bounds, nu, flags=torch.zeros((4, 100), dtype=torch.float32))
    with pytest.raises(ValueError, match="model"):
        lines.fit(x, bounds, nu, model=torch.zeros((4, 99), dtype=torch.float32))
    with pytest.raises(ValueError, match="min_hits"):
        lines.fit(x, bounds, nu, min_hits=-1)
    with pytest.raises(ValueError, match="rcond"):
        lines.fit(x, bounds, nu, rcond=1.0)
    for v in (a.float(), a[:, :1], torch.zeros((4, 2, 6), dtype=torch.float64), a.numpy()):
        with pytest.raises(ValueError, match="a must"):
            lines.apply(x, bounds, nu, v, 1)
    with pytest.raises(ValueError, match="sign"):
        lines.apply(x, bounds, nu, a, 1, sign=0)
    with pytest.raises(ValueError, match="out"):
        lines.apply(x, bounds, nu, a, 1, out=torch.zeros((4, 99), dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be x or must not overlap"):
        lines.apply(x[:, :99], np.array([0, 50, 99]), nu, a, 1, out=x[:, 1:])
    with pytest.raises(ValueError, match="n_iter"):
        lines.refine(x, bounds, nu, n_iter=-1)
    # a host tensor gets every other refusal first, then this one: no quiet fall-back to the host
    with pytest.raises(ValueError, match="device tensor"):
        lines.normal_equations(x, bounds, nu)
    with pytest.raises(ValueError, match="device tensor"):
        lines.apply(x, bounds, nu, a, 1)
    with pytest.raises(ValueError, match="device tensor"):
        lines.inject_lines(x, [7.0], [1.0], [0.0], 100.0)
    for args in (([7.0], [1.0, 2.0], [0.0], 100.0), ([7.0], [1.0], [0.0], 0.0), ([60.0], [1.0], [0.0], 100.0), ([], [], [], 100.0)):
        with pytest.raises(ValueError):
            lines.inject_lines(x, *args)
    for v, n_poly in ((np.zeros((2, 3, 4)), 1), (np.zeros((2, 3, 1)), 1), (np.zeros((2, 3, 10)), 2), (np.zeros((2, 3)), 0)):
        with pytest.raises(ValueError):
            lines.amplitude_phase(v, n_poly)
    f, p = np.arange(200.0), np.ones((3, 200))
    for kw in (dict(half_window=0), dict(half_window=60), dict(n_sigma=0.0), dict(max_lines=-1), dict(groups=[0, 1]), dict(groups=[0, -2, 0])):
        with pytest.raises(ValueError):
            lines.find_lines(f, p, **kw)
    with pytest.raises(ValueError):
        lines.find_lines(f[:-1], p)
    with pytest.raises(ValueError):
        lines.find_lines(f[::-1], p)
    assert lines.MAX_LINES == 3 and lines.MAX_POLY == 2
    assert [list(g) for g in lines.line_groups(7)] == [[0, 1, 2], [3, 4, 5], [6]] and lines.line_groups(0) == []


def host_tod(D=4, T=4096, fs=100.0):
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    dets = Detectors(np.zeros((D, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int))
    t = 1.7e9 + np.arange(T) / fs
    return TOD({"signal": np.zeros((D, T), np.float32)}, dets, Coordinates(t, np.zeros(T), np.full(T, 1.0)), units="K_RJ")


def test_tod_remove_lines_refusals():
    """Everything TOD.remove_lines refuses before it touches a device."""
    tod = host_tod()
    for kw in (dict(n_poly=3), dict(n_poly=-1), dict(min_hits=-1), dict(rcond=1.0), dict(n_refine=-1), dict(n_refine=1.5), dict(n_sigma=0.0),
               dict(n_sigma=float("nan")), dict(nperseg=1000), dict(nperseg=8192), dict(chunk=0.0), dict(chunk=float("inf")),
               dict(chunk=30.0), dict(nperseg=256, chunk=5.0), dict(groups="array"), dict(groups=np.zeros((2, 2), int)), dict(into="nothing")):
        with pytest.raises(ValueError):
            tod.remove_lines(**kw)
    import inspect

    from maria_amd.sim import TOD

    sig = inspect.signature(TOD.remove_lines)
    assert list(sig.parameters)[1:] == ["lines", "chunk", "n_poly", "n_sigma", "nperseg", "n_refine", "per_detector", "groups", "model", "into",
                                        "min_hits", "rcond", "ctx", "device"]
    assert sig.parameters["n_poly"].default == 2 and sig.parameters["n_sigma"].default == 6.0 and sig.parameters["n_refine"].default == 2
    assert "flag_glitches" in TOD.remove_lines.__doc__ and "remove_common_mode" in TOD.remove_lines.__doc__


# ---- the finder ----

def science_spectrum(clean=False):
    import scipy.signal

    x, free, hz, _ = ref.science_case()
    return scipy.signal.welch((free if clean else x).astype(np.float64), ref.FS, nperseg=2048)


def test_find_lines_finds_the_injected_set_and_nothing_else():
    f, p = science_spectrum()
    (got,), (want,) = lines.find_lines(f, p), ref.find_lines(f, p)
    assert got.size == 2 and np.array_equal(got, want)
    assert np.abs(got - np.array(ref.LINE_HZ)).max() < 0.5 * ref.FS / 2048  # strongest first: the order of LINE_HZ
    assert lines.find_lines(f, p, max_lines=1)[0].tolist() == got[:1].tolist()
    assert lines.find_lines(f, p, f_min=10.0)[0].tolist() == got[1:].tolist() and lines.find_lines(f, p, f_max=10.0)[0].tolist() == got[:1].tolist()
    # two groups, a row in none: each group its own list; tensors are taken too
    import torch

    g = np.array([0] * 6 + [1] * 5 + [-1])
    both = lines.find_lines(torch.as_tensor(f), torch.as_tensor(p), groups=g)
    assert len(both) == 2 and all(v.size == 2 and np.abs(v - got).max() < 0.01 for v in both)
    assert all(np.array_equal(a, b) for a, b in zip(both, ref.find_lines(f, p, groups=g)))


def test_find_lines_on_red_noise_without_lines_gives_none():
    f, p = science_spectrum(clean=True)
    assert p[:, 1].mean() > 30 * np.median(p, axis=1).mean()  # the 1 / f^2 drift is there
    assert lines.find_lines(f, p)[0].size == 0 and ref.find_lines(f, p)[0].size == 0
    # a pure power law with the scatter of a Welch average, steeper and without a white floor
    rng = np.random.default_rng(3)
    f = np.arange(1025) * (100.0 / 2048)
    p = (1.0 + (1.0 / np.maximum(f, f[1])) ** 2.5)[None, :] * rng.chisquare(40, (12, 1025)) / 40
    assert lines.find_lines(f, p)[0].size == 0 and ref.find_lines(f, p)[0].size == 0


def test_find_lines_leaves_out_the_ends_of_the_spectrum():
    rng = np.random.default_rng(4)
    F, h = 1025, 16
    f = np.arange(F) * (100.0 / 2048)
    p = rng.chisquare(40, (12, F)) / 40
    for k in (3, h - 2, F - h + 1, F - 2):  # inside the excluded first and last half_window bins
        p[:, k] *= 50.0
    assert lines.find_lines(f, p)[0].size == 0 and ref.find_lines(f, p)[0].size == 0
    for k in (h, 500, F - h - 1):  # the first and the last bins that count, and one between
        p[:, k] *= 50.0
    (got,) = lines.find_lines(f, p)
    assert sorted(np.round(got / f[1]).astype(int).tolist()) == [h, 500, F - h - 1] and np.array_equal(got, ref.find_lines(f, p)[0])
    assert sorted(np.round(lines.find_lines(f, p, half_window=8)[0] / f[1]).astype(int).tolist()) == [h - 2, h, 500, F - h - 1, F - h + 1]


# ---- the refinement ----

def test_refine_converges_from_half_a_bin():
    """Noise-free lines, every detector's frequency half a Welch bin (of 2048 samples) off, chunks of 1024 samples (a
    quarter of a cycle of slip a chunk): a line's fitted phase is the true one at the chunk's centre up to terms of
    second order in the slip, so the first round leaves a few per cent of the error and the second less than 1e-3 of it."""
    D, T, n = 4, 16384, 1024
    rng = np.random.default_rng(6)
    true = np.array([0.073137, 0.21947])[None, :] * (1 + 1e-4 * rng.standard_normal((D, 2)))
    t = np.arange(T)
    x = sum(a * np.cos(2 * np.pi * true[:, l, None] * t[None, :] + rng.uniform(-3, 3, (D, 1))) for l, a in enumerate((0.5, 0.3))).astype(np.float32)
    bounds = ref.chunk_bounds(T, n)
    off = 0.5 / 2048
    start = true + off * np.array([1.0, -1.0])[None, :]
    one = ref.refine(x, bounds, start, n_iter=1, n_poly=2, fit=ref.fit_fast)
    two = ref.refine(x, bounds, start, n_iter=2, n_poly=2, fit=ref.fit_fast)
    e1, e2 = np.abs(one - true).max() / off, np.abs(two - true).max() / off
    print(f"error / half a bin after one round {e1:.2e}, after two {e2:.2e}")
    assert e1 < 0.1 and e2 < 1e-3
    # one correction for all rows: the median of theirs
    step = ref.refine(x, bounds, start, n_iter=1, n_poly=2, per_detector=False, fit=ref.fit_fast) - start
    assert np.all(step == step[:1]) and np.abs(step[0] + off * np.array([1.0, -1.0])).max() < 0.1 * off


def test_phase_slope_against_the_reference_and_its_exclusions():
    rng = np.random.default_rng(8)
    D, S, n_poly, L = 5, 9, 1, 2
    bounds = np.array([0, 100, 100, 250, 400, 520, 700, 800, 950, 1000], np.int32)  # one empty segment
    a = rng.standard_normal((D, S, n_poly + 2 * L))
    ok = rng.random((D, S)) < 0.8
    ok[3] = False  # a row without any pair: no correction
    ok[4, ::2] = False  # a row whose fitted segments are never neighbours
    groups = np.array([0, 0, 1, 1, -1])
    for per_detector in (True, False):
        got = lines.phase_slope(a, ok, bounds, 1000, n_poly, groups=groups, per_detector=per_detector)
        want = ref.phase_slope(a, ok, bounds, 1000, n_poly, groups=groups, per_detector=per_detector)
        assert got.shape == (D, L) and np.array_equal(got, want)
    assert not lines.phase_slope(a, ok, bounds, 1000, n_poly)[3].any()
    # a known slope: phases 2 pi dnu c_s, wrapped, come back as dnu
    centre = lines.segment_centres(bounds, 1000)[0]
    dnu = 2.5e-3  # 150 samples between centres at the most: 0.375 cycles
    phi = 2 * np.pi * dnu * centre
    a = np.zeros((1, S, 2))
    a[0, :, 0], a[0, :, 1] = np.cos(phi), -np.sin(phi)
    assert abs(lines.phase_slope(a, np.ones((1, S), bool), bounds, 1000, 0)[0, 0] - dnu) < 1e-15


# ---- the science fixture on the host ----

def test_the_reference_pipeline_cleans_the_science_fixture_near_the_noise_floor():
    """D = 12, T = 24 000 at 100 Hz, lines of 0.5 and 0.3 sigma at 7.3137 and 21.947 Hz scattered by 1e-4 between the
    detectors, on white noise and a random walk.  Found: exactly the two.  Refined: within 7e-4 Hz of every detector's
    own.  Residual (cleaned less line-free, over the injected rms) <= 1.5 x the floor of 2 L amplitudes a chunk,
    sigma sqrt(2 L S / T) / injected rms; measured 0.110 = 1.02 x the floor 0.108."""
    x, clean, hz, rms = ref.science_case()
    D, T = x.shape
    y, rec = ref.remove_lines(x, x, ref.FS, nperseg=2048)
    assert rec["lines"][0].size == 2 and rec["unfitted"] == 0
    err = np.abs(rec["refined"] - hz).max()
    floor = ref.noise_floor(2, ref.chunk_bounds(T, 2048), T, 1.0, rms)
    resid = math.sqrt(((y.astype(np.float64) - clean) ** 2).mean()) / rms
    print(f"max |refined - true| = {err:.2e} Hz; residual {resid:.4f} of the injected rms = {resid / floor:.3f} x the floor {floor:.4f}")
    assert err <= 7e-4
    assert 0.9 * floor <= resid <= 1.5 * floor
    before = math.sqrt(((x.astype(np.float64) - clean) ** 2).mean()) / rms
    assert abs(before - 1.0) < 1e-6
    # the exact sums give the same frequencies as the fast ones the pipeline above uses, to rounding
    sub = slice(0, 2)
    a = ref.refine(x[sub], ref.chunk_bounds(T, 2048), rec["lines"][0] / ref.FS, n_poly=2, min_hits=24, fit=ref.fit)
    assert np.abs(a * ref.FS / rec["refined"][sub] - 1).max() < 1e-12


# ---- the mistakes the device bounds must see ----

def mistaken_sums(x, bounds, nu, n_poly, flags, model, mistake):
    """N and r (numpy sums) with one step of the basis done wrongly."""
    terms = ref._terms(x, model)
    D, T = terms.shape
    L = nu.shape[1]
    K = n_poly + 2 * L
    segs = ref.segments(bounds, T)
    N, r = np.zeros((D, len(segs), K, K)), np.zeros((D, len(segs), K))
    for s, (lo, hi) in enumerate(segs):
        for d in range(D if hi > lo else 0):
            B = ref.basis(lo, hi, nu[d], n_poly)
            t = np.arange(lo, hi)
            if mistake == "segment start":
                B[n_poly:] = ref.basis(0, hi - lo, nu[d], 0)
            elif mistake == "float32 theta":
                theta = (nu[d].astype(np.float32)[:, None] * t.astype(np.float32)[None, :]).astype(np.float64)
                sn, cs = ref.sincospi(2.0 * (theta - np.rint(theta)))
                B[n_poly::2], B[n_poly + 1::2] = cs, sn
            elif mistake == "cos(2 pi q)":
                q = ref.reduced_phase(nu[d], t)
                B[n_poly::2], B[n_poly + 1::2] = np.cos(2 * np.pi * q), np.sin(2 * np.pi * q)
            y = terms[d, lo:hi]
            if mistake == "times zero":
                w = (flags[d, lo:hi] == 0).astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    N[d, s], r[d, s] = ((B * w)[:, None, :] * B[None, :, :]).sum(axis=2), ((B * w) * y[None, :]).sum(axis=1)
                continue
            keep = np.ones(hi - lo, bool) if flags is None else flags[d, lo:hi] == 0
            b, y = B[:, keep], y[keep]
            N[d, s], r[d, s] = (b[:, None, :] * b[None, :, :]).sum(axis=2), (b * y[None, :]).sum(axis=1)
    return N, r


def test_the_mistakes_exceed_the_bounds_on_the_device_tests_inputs():
    """Gaussian rows with generic frequencies (test_gpu_lines.py: test_sums_within_the_bound): the phase taken from the
    segment's start and a float32 theta move N and r far outside the bound.  Small integers at 1/4 and 1/2 cycle a sample
    with 1e30 and NaN under the flags (its bit-for-bit cases): cos(2 pi q) in place of cospi and a flagged sample
    multiplied by zero change bits."""
    D, T, n_poly, L = 3, 1025, 2, 3
    bounds = make_bounds(T, 10 * (n_poly + 2 * L) + T)
    x, model, flags = rows(D, T, 1000 * T + 10 * D + n_poly + 2 * L, exact=False)
    nu = generic_nu(D, L, T + D)
    N, r, hits, aN, ar, dN, dr = ref.normal_equations(x, bounds, nu, n_poly, flags=flags, model=model)
    bN, br = sum_bounds(bounds, aN, ar, dN, dr)
    late = bounds[:-1] > 0
    for mistake, least in (("segment start", 1e9), ("float32 theta", 1e6)):
        Nm, rm = mistaken_sums(x, bounds, nu, n_poly, flags, model, mistake)
        full = np.flatnonzero(late & (np.diff(bounds) >= 63))
        over = np.abs(rm - r)[:, full][:, :, n_poly:] / br[:, full][:, :, n_poly:]
        print(f"{mistake}: |r - ref| / bound on the segments of 63 samples and more: median {np.median(over):.3g}")
        assert np.median(over) > least
        assert (np.abs(Nm - N) > bN).any()
    right = mistaken_sums(x, bounds, nu, n_poly, flags, model, None)
    assert np.all(np.abs(right[0] - N) <= bN) and np.all(np.abs(right[1] - r) <= br)  # the harness itself is inside
    # the bit-for-bit inputs
    x, model, flags = rows(D, T, 3, exact=True)
    nu = quarter_nu(D, L)
    N, r = ref.normal_equations(x, bounds, nu, n_poly, flags=flags, model=model)[:2]
    same = mistaken_sums(x, bounds, nu, n_poly, flags, model, None)
    carriers = (slice(None), slice(None), slice(n_poly, None))
    assert np.array_equal(same[1][carriers], r[carriers]) and np.array_equal(same[0][carriers + (slice(n_poly, None),)], N[carriers + (slice(n_poly, None),)])
    wrong = mistaken_sums(x, bounds, nu, n_poly, flags, model, "cos(2 pi q)")  # a sum of exact zeros, cos sin at 1/4, is one no more
    assert not np.array_equal(wrong[0][carriers + (slice(n_poly, None),)], N[carriers + (slice(n_poly, None),)])
    for fill in (1e30, np.nan):
        dirty = x.copy()
        dirty[flags != 0] = fill
        assert np.array_equal(ref.normal_equations(dirty, bounds, nu, n_poly, flags=flags, model=model)[1], r)
        wrong = mistaken_sums(dirty, bounds, nu, n_poly, flags, model, "times zero")
        assert np.isnan(fill) == (not np.array_equal(wrong[1][carriers], r[carriers]))  # 0 * 1e30 is 0, 0 * NaN is not
