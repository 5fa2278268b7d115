"""Every TOD entry of include/mrx.h that takes a row pitch, on rows that start past 2^31 and 2^32 elements.

The layout is tests/wide_rows.py's: three rows of a few thousand samples at a pitch of 2^31 + 4 ("aligned") or 2^31 + 5
elements, one element in ("odd"), in one arena of 17.2 GB of which only the rows and their guard strips are touched.  For
every entry of TABLE, every pitched role (a pitch argument and the arrays it governs) and both pitches one call is made with
that role wide and everything else compact, and:

  1. every output equals, in every bit, the same entry's output on contiguous copies of the same data (the entries that
     add with atomics get data on a power-of-two grain: their float64 sums are exact in any order);
  2. the outputs meet the float64 reference of the entry's own test file under that file's own acceptance (the bounds and
     builders are imported from there);
  3. the wide array's guard strips, the compact arrays' padding and the inputs are untouched.

test_a_wrong_pitch_is_noticed makes one more call per entry and role, handing the entry the compact pitch T + 128 for the
wide array: every access then stays inside the arena's sentinel-filled head, rows 1 and 2 are read or written at the wrong
place, and 1 or 3 must fail.  No kernel is mutated for this: a truncated row offset would fault the card.

Where a maria_amd wrapper takes pitched views for every pitched role of its entry the call goes through it (its pitch
arithmetic and torch operations are then under test too: 27 entries); the others are called through Context.call: an
output the wrapper allocates itself (mrx_tod_column_mean's mean, mrx_tod_column_fit's and _apply's c), outputs that share a
pitch and would be refused as overlapping when they are slots of one arena (mrx_tod_demodulate), entries whose wrapper does
more than the entry (mrx_tod_glitch_flag, mrx_tod_jump_find, the pre-processing, K_RJ and map entries).

The three rows hold different data; row lists and groups name the rows out of order.  T is the smallest length at which an
entry's kernel takes every path: two full work items and a ragged remainder that is no multiple of 4."""

import ctypes as C
import functools
import time
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import wide_rows as wr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = wr.D
T0 = 2 * 1024 + 37
T_MAX = 8800  # the longest row of a case below (mrx_tod_segment_flag: 2 x 4096 + 517)
ORDER = np.array([2, 0, 1], np.int32)  # row lists and groups: out of order

# Entries with a pitch argument that this module leaves out, and why (tests/test_host_wide_rows.py holds the two lists
# against the header).
SIMULATION = ("the simulation's writers and samplers run at 10 000 x 240 000 in tests/test_gpu_fullsize.py; rows past 2^32 "
              "elements are a follow-up")
SAME_READER = "its only pitch is ld_weight, read by the code that reads mrx_bin_map's"
EXCLUDED = {
    **{name: SIMULATION for name in (
        "mrx_spline_upsample", "mrx_spline_upsample_fused", "mrx_spline_upsample_krj", "mrx_atm_synthesize", "mrx_atm_synthesize_krj",
        "mrx_coarse_to_krj_keep_tail", "mrx_pointing_broadcast", "mrx_linear_upsample", "mrx_resample_columns", "mrx_map_sample",
        "mrx_map_sample_krj", "mrx_noise_generate", "mrx_noise_generate_krj")},
    **{name: SAME_READER for name in ("mrx_bin_map_bucketed", "mrx_map_normal_apply", "mrx_bin_map_blocks", "mrx_bin_map_baselines")},
}
# Not covered either, by construction of the cases: rows longer than 2^24 samples, and D x S or D x tiles past 2^31 work items.


# ---- the engine ----

class A:
    """One array of a case: host data, "in" | "out" | "inout", and the pitch argument(s) that govern it ("ld_x"; an array
    handed over twice, in place, "ld_x+ld_y"; None: not pitched)."""

    def __init__(self, data, role, ld=None):
        self.data, self.role, self.ld = np.ascontiguousarray(data), role, ld
        self.data.setflags(write=False)


def I(data, ld=None):  # noqa: E741, E743
    return A(data, "in", ld)


def O(shape, dtype, ld=None, fill=7):  # noqa: E741, E743
    return A(np.full(shape, fill, dtype), "out", ld)


def IO(data, ld=None):
    return A(data, "inout", ld)


class Case:
    """arrays: name -> A, in the order of no importance; call(ctx, v, ld) with v.name the device tensors and ld.name the
    pitches (it may return {name: tensor} of further outputs); check(out) asserts out.name against the reference."""

    def __init__(self, arrays, call, check):
        self.arrays, self.call, self.check = arrays, call, check

    def roles(self):
        return sorted({a.ld for a in self.arrays.values() if a.ld})


def nothing(*_):
    """(A wrapper's return value, the tensor it was given as ``out``, is no further output.)"""
    return None


def P(t):
    from maria_amd._lib import ptr

    return ptr(t)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def on_device(a):
    import torch

    with warnings.catch_warnings():  # the cases are read-only arrays; they are only read here
        warnings.simplefilter("ignore", UserWarning)
        return torch.as_tensor(a).to(DEV)


def all_are(t, fill):
    import torch

    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


class Compact:
    """A [rows, T] array at the compact pitch T + 2 GUARD, GUARD elements into a sentinel-filled buffer of its own."""

    def __init__(self, a):
        import torch

        rows, T = a.shape
        self.fill, self.geom = wr.sentinel(a.dtype), ((rows, T), (wr.compact_pitch(T), 1), wr.GUARD)
        self.buf = torch.full((rows * wr.compact_pitch(T) + wr.GUARD,), self.fill, dtype=on_device(a[:0]).dtype, device=DEV)
        self.view = torch.as_strided(self.buf, *self.geom)
        self.view.copy_(on_device(a))

    def padding_intact(self):
        import torch

        rest = self.buf.clone()
        torch.as_strided(rest, *self.geom).fill_(self.fill)
        return all_are(rest, self.fill)


def run(ctx, case, arena=None, role=None, layout=None, wrong=False):
    """One call of the case.  role None: every array contiguous (the baseline).  Else the arrays of ``role`` wide in the
    arena at ``layout`` and the other pitched ones compact; ``wrong``: the entry is handed the compact pitch for the wide
    arrays (views of the arena's head), and the results are read where a right call would have put them.
    Returns (outputs name -> host array, nothing written outside the rows, inputs unchanged)."""
    import torch

    v, true, compact = {}, {}, []
    wide = [n for n, a in case.arrays.items() if role is not None and a.ld == role]
    if wide:
        views, _ = arena.place([case.arrays[n].data for n in wide], layout)
        true = dict(zip(wide, views))
    for name, a in case.arrays.items():
        if name in true:
            v[name] = true[name]
            if wrong:
                T, size = a.data.shape[1], a.data.dtype.itemsize
                v[name] = torch.as_strided(arena.placed[0], (D, T), (wr.compact_pitch(T), 1), wr.row_start(layout, size, T, 0, wide.index(name)))
        elif a.ld is None or role is None:
            v[name] = on_device(a.data)
        else:
            compact.append(Compact(a.data))
            v[name] = compact[-1].view
    ld = {}
    for name, a in case.arrays.items():
        for token in (a.ld or "").split("+"):
            if token:
                pitch = v[name].stride(0)
                assert ld.setdefault(token, pitch) == pitch, f"{token}: two arrays of one pitch argument at different pitches"
    more = case.call(ctx, SimpleNamespace(**v), SimpleNamespace(**ld))
    torch.cuda.synchronize()
    out = {n: true.get(n, v[n]).cpu().numpy() for n, a in case.arrays.items() if a.role != "in"}
    out.update({n: t.cpu().numpy() for n, t in (more or {}).items()})
    unchanged = all(same_bits(true.get(n, v[n]).cpu().numpy(), a.data) for n, a in case.arrays.items() if a.role == "in")
    intact = all(c.padding_intact() for c in compact) and (not wide or arena.guards_intact())
    return out, intact, unchanged


def differing(out, base):
    return [n for n in base if not same_bits(out[n], base[n])]


def exact(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.dtype != want.dtype:  # counts: the device's uint32 against the reference's int64
        assert np.array_equal(got.astype(np.int64), want.astype(np.int64)), int((got != want).sum())
    else:
        assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


def rows3(T, seed, scale=3.0, offset=5.0):
    return (np.random.default_rng(seed).standard_normal((D, T)) * scale + offset).astype(np.float32)


# ---- spectra, noise filters ----

def welch(ctx):
    from test_gpu_noise_estimate import _check, _reference, _rows

    from maria_amd import noise_estimate

    n, fs = 256, 37.0
    T = n + 16 * (n // 2) + 37  # 17 segments: a full batch of eight pairs and an unpaired one; 37 trailing samples dropped
    x = _rows(T, fs, n, np.random.default_rng(n))[1:]  # 1/f, a sinusoid, white on an offset of 1e4
    want = _reference(x, fs, n)
    return Case(dict(x=I(x, "ld")), lambda c, v, ld: dict(psd=noise_estimate.welch(v.x, fs, nperseg=n, ctx=c)[1]),
                lambda o: _check(o["psd"], want, "wide rows"))


def _filter_inputs(K, m):
    from test_gpu_noise_filter import _lags

    T = 2 * (4096 - 2 * K) + 37  # two overlap-save blocks of the 4096-point transform and a remainder
    rng = np.random.default_rng(K + m)
    x = (rng.normal(size=(D, T)) * rng.uniform(0.1, 10.0, (D, 1))).astype(np.float32)
    x[0] += 50.0
    k = _lags(D, K, rng)
    sw = rng.uniform(0.0, 1.5, (D, T)).astype(np.float32)
    U = rng.normal(size=(D, max(m, 1)))
    b = (rng.normal(size=(max(m, 1), T)) * 3.0).astype(np.float32)
    return T, x, k, sw, U, b


def _filter_check(got, ref, mag):
    from test_gpu_noise_filter import ROW_TOL

    err = np.abs(got - ref).max(axis=1) / np.maximum(mag, 1e-300)
    assert err.max() <= ROW_TOL, (err.max(), int(err.argmax()))


def noise_filter(ctx):
    from test_gpu_noise_filter import _reference

    from maria_amd import noise_filter

    K = 16
    T, x, k, sw, _, _ = _filter_inputs(K, 0)
    ref, mag = _reference(x, k, sw.astype(np.float64))
    return Case(dict(x=I(x, "ld_x"), y=O((D, T), np.float32, "ld_y"), lags=I(k), sw=I(sw, "ld_w")),
                lambda c, v, ld: nothing(noise_filter.apply(c, v.x, v.lags, v.sw, out=v.y)),
                lambda o: _filter_check(o["y"], ref, mag))


def noise_filter_modes(ctx):
    from test_gpu_noise_modes import _reference

    from maria_amd import noise_modes

    K, m = 16, 2
    T, x, k, sw, U, b = _filter_inputs(K, m)
    s, b64 = sw.astype(np.float64), b.astype(np.float64)
    ref, _ = _reference(x.astype(np.float64) - U @ b64, k, s)
    _, mag = _reference(np.abs(x).astype(np.float64) + np.abs(U) @ np.abs(b64), k, s)
    return Case(dict(x=I(x, "ld_x"), y=O((D, T), np.float32, "ld_y"), lags=I(k), sw=I(sw, "ld_w"), U=I(U), b=I(b)),
                lambda c, v, ld: nothing(noise_modes.filter_modes(c, v.x, v.lags, v.sw, v.U, v.b, v.y)),
                lambda o: _filter_check(o["y"], ref, mag))


def mode_project(ctx):
    from maria_amd import noise_modes

    T, m = T0, 5
    rng = np.random.default_rng(m)
    x = (rng.normal(size=(D, T)) * rng.uniform(0.1, 10.0, (D, 1)) + 3.0).astype(np.float32)
    U = rng.normal(size=(D, m))
    xs = x.astype(np.float64)
    ref, mag = U.T @ xs, np.abs(U).T @ np.abs(xs)

    def check(o):
        err = float((np.abs(o["a"] - ref) / mag).max())
        assert err <= 1e-13, err  # tests/test_gpu_noise_modes.py: test_mode_project_matches_float64

    return Case(dict(x=I(x, "ld_x"), U=I(U), a=O((m, T), np.float64)),
                lambda c, v, ld: nothing(noise_modes.project(c, v.x, v.U, out=v.a)), check)


# ---- decimation, glitches, jumps ----

def decimate(ctx):
    from test_gpu_resident_trips import decimate_case

    from maria_amd import downsample

    q, n_taps = 3, 41
    T_out = 2 * downsample.TILE_OUTPUTS + 37
    T = q * T_out - 1
    assert downsample.output_length(T, q) == T_out
    x, h, want, tol = decimate_case(D, T, q, n_taps)

    def check(o):
        worst = float((np.abs(o["y"].astype(np.float64) - want) / tol).max())
        assert worst <= 1.0, worst

    def call(c, v, ld):
        assert downsample.decimate(v.x, q, taps=h, ctx=c, out=v.y) is v.y

    return Case(dict(x=I(x, "ld_x"), y=O((D, T_out), np.float32, "ld_y")), call, check)


def median_residual(ctx):
    from test_gpu_resident_trips import HALF, T3, glitch_case

    from maria_amd import flagging

    x, _, want, _, _ = glitch_case(D)

    def call(c, v, ld):
        assert flagging.median_residual(v.x, HALF, ctx=c, out=v.r) is v.r

    return Case(dict(x=I(x, "ld_x"), r=O((D, T3), np.float32, "ld_r")), call, lambda o: exact(o["r"], want))


def glitch_flag(ctx):
    from test_gpu_resident_trips import GROW, HALF, T3, glitch_case

    x, thresh, _, want, n_want = glitch_case(D)

    def check(o):
        exact(o["flags"], want)
        exact(o["count"], n_want)

    return Case(dict(x=I(x, "ld_x"), thresh=I(thresh), flags=O((D, T3), np.uint8, "ld_f", 9), count=O((D,), np.int32, fill=12345)),
                lambda c, v, ld: c.call("mrx_tod_glitch_flag", P(v.x), ld.ld_x, D, T3, HALF, P(v.thresh), GROW[0], GROW[1], P(v.flags), ld.ld_f,
                                        P(v.count)), check)


def gap_fill(ctx):
    from test_gpu_resident_trips import N_FIT, fill_case

    from maria_amd import flagging

    x, f, want, n_want, scale = fill_case(D)

    def check(o):
        keep = (f == 0) | (np.arange(D) % 5 == 2)[:, None]
        assert np.array_equal(o["x"][keep], x[keep]), "an unflagged sample, or a row flagged end to end, changed"
        err = np.abs(o["x"].astype(np.float64) - want)
        assert float((err[~keep] / (2.0**-23 * scale[~keep])).max()) <= 1.0
        exact(o["filled"], n_want)

    return Case(dict(x=IO(x, "ld_x"), flags=I(f, "ld_f")), lambda c, v, ld: dict(filled=flagging.gap_fill(v.x, v.flags, N_FIT, ctx=c)), check)


def step_stat(ctx):
    from test_gpu_resident_trips import GAP, T3, WINDOW, stat_case

    from maria_amd import jumps

    x, f, want, _ = stat_case(D, True)  # rows of small integers: bit for bit

    def call(c, v, ld):
        assert jumps.step_statistic(v.x, WINDOW, GAP, flags=v.flags, min_count=WINDOW // 2, ctx=c, out=v.s) is v.s

    return Case(dict(x=I(x, "ld_x"), flags=I(f, "ld_f"), s=O((D, T3), np.float32, "ld_s")), call, lambda o: exact(o["s"], want))


def jump_find(ctx):
    import jumps_ref
    from test_gpu_jumps import find_case
    from test_gpu_resident_trips import SEP, T3

    s, thresh = find_case(D, T3, SEP, seed=D)
    want, n_want = jumps_ref.find(s, thresh, SEP, 4, 64)
    assert n_want[0] >= 3 and n_want[2] >= 3 and n_want[1] == 0

    def check(o):
        exact(o["flags"], want)
        exact(o["count"], n_want)

    return Case(dict(s=I(s, "ld_s"), thresh=I(thresh), flags=O((D, T3), np.uint8, "ld_f", 9), count=O((D,), np.int32, fill=12345)),
                lambda c, v, ld: c.call("mrx_tod_jump_find", P(v.s), ld.ld_s, D, T3, P(v.thresh), SEP, 4, 64, P(v.flags), ld.ld_f, P(v.count)),
                check)


def jump_height(ctx):
    import jumps_ref
    from test_gpu_jumps import positive_rows

    from maria_amd import jumps

    w, g = 32, 4
    x, f = positive_rows(D, T0, seed=11, integers=True)  # small integers: the float64 means are exact
    f[1] = np.roll(f[2], 7)  # (positive_rows flags row 1 end to end)
    lists = [[300, 900, 1023, 1500], [40, 1024, 1030, 2000], [5, 1100, T0 - 3]]
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int32)
    pos = np.asarray([p for r in lists for p in r], np.int32)
    want, ok_want = jumps_ref.heights(x, row_start, pos, w, g, f)
    assert ok_want.sum() >= 6 and all(ok_want[row_start[d]:row_start[d + 1]].any() for d in range(D))

    def call(c, v, ld):
        height, ok = jumps.jump_heights(v.x, row_start, pos, w, g, flags=v.flags, ctx=c)
        return dict(height=height, ok=ok)

    def check(o):
        assert np.array_equal(o["ok"], ok_want)
        exact(o["height"], want)

    return Case(dict(x=I(x, "ld_x"), flags=I(f, "ld_f")), call, check)


def jump_fix(ctx):
    import jumps_ref
    from test_gpu_resident_trips import T3, TILE

    from maria_amd import jumps

    s, T = TILE, T3
    rng = np.random.default_rng(D + 1)
    x = (rng.standard_normal((D, T)) * 3 + np.linspace(-20.0, 20.0, T)).astype(np.float32)
    lists = [[0, 77, 77, s - 1, s, 2 * s - 1, 2 * s, T - 1], [int(rng.integers(0, T))], sorted(rng.choice(T, 40, replace=False).tolist())]
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int32)
    pos = np.asarray([p for r in lists for p in r], np.int32)
    heights = rng.uniform(-16.0, 16.0, pos.size)
    want = jumps_ref.fix(x, row_start, pos, jumps_ref.cumulative(row_start, heights))

    def call(c, v, ld):
        assert jumps.fix_jumps(v.x, row_start, pos, heights, out=v.y, ctx=c) is v.y

    return Case(dict(x=I(x, "ld_x"), y=O((D, T), np.float32, "ld_y")), call, lambda o: exact(o["y"], want))


# ---- ground, regression, sky polynomials ----

def bin_reduce(ctx):
    import ground_ref
    from test_gpu_ground import SIZES, keys, rows

    from maria_amd import ground

    K, T, min_hits = 11, T0, 8
    b = keys(T, K, D, absent=True)
    assert np.bincount(b[b >= 0], minlength=K)[:6].tolist() == SIZES
    x, model, flags = rows(D, T, D + 1, exact=True)
    s_ref, h_ref, t_ref, _ = ground_ref.bin_reduce(x, b, K, flags=flags, model=model, min_hits=min_hits)

    def check(o):
        exact(o["hits"], h_ref)
        exact(o["sums"], s_ref)
        exact(o["tmpl"], t_ref)

    def call(c, v, ld):
        tmpl, hits, sums = ground.bin_template(v.x, b, K, flags=v.flags, model=v.model, min_hits=min_hits, ctx=c)
        return dict(tmpl=tmpl, hits=hits, sums=sums)

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f")), call, check)


def bin_apply(ctx):
    import ground_ref

    from maria_amd import ground

    K, T, sign = 360, T0, -1
    rng = np.random.default_rng(D + K)
    x = rows3(T, D + K)
    tmpl = rng.standard_normal((D, K)).astype(np.float32)
    b = rng.integers(-1, K, T).astype(np.int32)  # -1: in no bin
    want = ground_ref.bin_apply(x, b, tmpl, sign)

    def call(c, v, ld):
        assert ground.apply_template(v.x, b, v.tmpl, sign, out=v.y, ctx=c) is v.y

    return Case(dict(x=I(x, "ld_x"), tmpl=I(tmpl), y=O((D, T), np.float32, "ld_y")), call, lambda o: exact(o["y"], want))


def _regress_rows(seed):
    """(x, model, flags, u, v, off) on small integers (every sum exact), v > 0; one row a group, named out of order."""
    from test_gpu_regress import rows

    x, model, flags, u, v, off = rows(D, T0, seed, True)
    return x, model, flags, u, np.maximum(v, 1.0), off


def column_mean(ctx):
    import regress_ref

    G, T = D, T0
    x, model, flags, u, v, off = _regress_rows(21)
    S_ref, W_ref, m_ref, _ = regress_ref.column_mean(x, u, v, off=off, groups=ORDER, n_groups=G, flags=flags, model=model)
    assert W_ref.all(axis=0).any() and not W_ref.all()

    def check(o):
        exact(o["S"], S_ref)
        exact(o["W"], W_ref)
        exact(o["mean"], m_ref)

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f"), groups=I(ORDER), u=I(u), v=I(v), off=I(off),
                     S=O((G, T), np.float64), W=O((G, T), np.float64), mean=O((G, T), np.float32, "ld_c")),
                lambda c, v_, ld: c.call("mrx_tod_column_mean", P(v_.x), ld.ld_x, P(v_.model), ld.ld_m, P(v_.flags), ld.ld_f, D, T, P(v_.groups), G,
                                         P(v_.u), P(v_.v), P(v_.off), P(v_.S), P(v_.W), P(v_.mean), ld.ld_c), check)


def _templates(seed):
    """B [G = 3][K = 1][T] of small integers: three template rows, one a group."""
    return np.random.default_rng(seed).integers(-8, 9, (D, 1, T0)).astype(np.float32)


def regress_normal(ctx):
    import regress_ref

    from maria_amd import regress

    G, K, T = D, 1, T0
    x, model, flags, _, _, _ = _regress_rows(22)
    B = _templates(23)
    N_ref, r_ref, h_ref, _, _ = regress_ref.normal_equations(x, B, groups=ORDER, flags=flags, model=model)

    def check(o):
        exact(o["hits"], h_ref)
        exact(o["N"], N_ref)
        exact(o["r"], r_ref)

    def call(c, v, ld):
        N, r, hits = regress.normal_equations(v.x, v.B.unsqueeze(1), groups=ORDER, flags=v.flags, model=v.model, ctx=c)
        return dict(N=N, r=r, hits=hits)

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f"), B=I(B.reshape(G * K, T), "ld_b")), call, check)


def regress_apply(ctx):
    import regress_ref

    from maria_amd import regress

    G, K, T, sign = D, 1, T0, -1
    x = rows3(T, 24)
    B = np.random.default_rng(25).standard_normal((G, K, T)).astype(np.float32)
    a = np.random.default_rng(26).standard_normal((D, K))
    want = regress_ref.apply(x, B, a, groups=ORDER, sign=sign)
    def call(c, v, ld):
        assert regress.apply(v.x, v.B.unsqueeze(1), v.a, groups=ORDER, sign=sign, out=v.y, ctx=c) is v.y

    return Case(dict(x=I(x, "ld_x"), B=I(B.reshape(G * K, T), "ld_b"), a=I(a), y=O((D, T), np.float32, "ld_y")), call, lambda o: exact(o["y"], want))


def column_fit(ctx):
    import skypoly_ref
    from test_gpu_skypoly import RATIO_MAX, U

    G, K, T = D, 1, T0  # three groups of one row: c [G][K][ld_c] is three rows
    x, model, flags, u, v, off = _regress_rows(27)
    u = np.where(u == 0, 1.0, u)
    Pm = np.ones((D, K))
    c_ref, ok_ref, h_ref, N_ref, r_ref, _ = skypoly_ref.fit(x, Pm, u, v, off=off, groups=ORDER, n_groups=G, flags=flags, model=model, min_hits=1)
    assert ok_ref.mean() > 0.9 and not ok_ref.all()

    def check(o):
        exact(o["hits"], h_ref)
        exact(o["N"], N_ref)
        exact(o["r"], r_ref)
        assert np.array_equal(o["ok"] != 0, ok_ref) and not o["c"].reshape(G, K, T)[:, 0][~ok_ref].any()
        # K = 1: cond(M) = 1, and the solve of the (exact) sums is held to the bound of test_gpu_skypoly.test_the_solve
        assert np.all(np.abs(o["c"].reshape(G, K, T) - c_ref) <= RATIO_MAX * U * np.abs(c_ref))

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f"), groups=I(ORDER), P=I(Pm), u=I(u), v=I(v), off=I(off),
                     c=O((G * K, T), np.float64, "ld_c"), ok=O((G, T), np.uint8, fill=9), hits=O((G, T), np.int32, fill=12345),
                     N=O((G, K * (K + 1) // 2, T), np.float64), r=O((G, K, T), np.float64)),
                lambda c, v_, ld: c.call("mrx_tod_column_fit", P(v_.x), ld.ld_x, P(v_.model), ld.ld_m, P(v_.flags), ld.ld_f, D, T, P(v_.groups), G,
                                         P(v_.P), K, P(v_.u), P(v_.v), P(v_.off), 1, 1e-10, P(v_.c), ld.ld_c, P(v_.ok), P(v_.hits), P(v_.N), P(v_.r)),
                check)


def column_apply(ctx):
    import skypoly_ref

    G, K, T, sign = D, 1, T0, -1
    rng = np.random.default_rng(28)
    x = rows3(T, 29)
    Pm = rng.integers(-4, 5, (D, K)) / 4.0 + 2.0
    c = rng.standard_normal((G, K, T))
    e, h = rng.standard_normal(D), rng.uniform(0.5, 2.0, D)
    want = skypoly_ref.apply(x, Pm, c, h, e=e, groups=ORDER, sign=sign)
    return Case(dict(x=I(x, "ld_x"), groups=I(ORDER), P=I(Pm), c=I(c.reshape(G * K, T), "ld_c"), e=I(e), h=I(h), y=O((D, T), np.float32, "ld_y")),
                lambda c_, v, ld: c_.call("mrx_tod_column_apply", P(v.x), ld.ld_x, D, T, P(v.groups), G, P(v.P), K, P(v.c), ld.ld_c, P(v.e), P(v.h),
                                          sign, P(v.y), ld.ld_y), lambda o: exact(o["y"], want))


# ---- subscans, lines, statistics, covariance ----

def segment_normal(ctx):
    import subscans_ref
    from test_gpu_subscans import HALF_ULP, make_bounds, rows

    from maria_amd import subscans

    K, T = 3, T0
    x, model, flags = rows(D, T, 31, exact=False)
    bounds = make_bounds(T, 31)
    flags[D - 1, bounds[2]:bounds[3]] = 2
    N_ref, r_ref, h_ref, aN, ar = subscans_ref.normal_equations(x, bounds, K, flags=flags, model=model)
    L = np.diff(bounds).astype(np.float64)
    bN, br = (L[None, :, None, None] + 1) * HALF_ULP * aN, (L[None, :, None] + 1) * HALF_ULP * ar

    def check(o):
        exact(o["hits"], h_ref)
        assert np.all(np.abs(o["N"] - N_ref) <= bN) and np.all(np.abs(o["r"] - r_ref) <= br)

    def call(c, v, ld):
        N, r, hits = subscans.normal_equations(v.x, bounds, K, flags=v.flags, model=v.model, ctx=c)
        return dict(N=N, r=r, hits=hits)

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f")), call, check)


def segment_apply(ctx):
    import subscans_ref
    from test_gpu_subscans import make_bounds

    from maria_amd import subscans

    K, T, sign = 4, T0, -1
    x = rows3(T, 32)
    bounds = make_bounds(T, 4)
    S = len(bounds) - 1
    a = np.random.default_rng(33).standard_normal((D, S, K))
    want = subscans_ref.apply(x, bounds, a, sign=sign)
    def call(c, v, ld):
        assert subscans.apply(v.x, bounds, v.a, sign, out=v.y, ctx=c) is v.y

    return Case(dict(x=I(x, "ld_x"), a=I(a), y=O((D, T), np.float32, "ld_y")), call, lambda o: exact(o["y"], want))


def segment_project(ctx):
    """tests/test_host_subscan_project.py's dense_case at this module's length: three segments of about 700 samples,
    30 % flagged, against the dense float64 operator under that case's bound."""
    import subscan_project_ref as pref
    import subscans_ref

    from maria_amd import subscans

    K, T, transpose = 3, T0, 0
    rng = np.random.default_rng(100 * K)
    bounds = np.array([2, 700, 1399, T - 3], np.int32)
    x = rows3(T, 34)
    flags = (rng.random((D, T)) < 0.3).astype(np.uint8)
    N, _, hits, _, _ = subscans_ref.normal_equations(x, bounds, K, flags=flags)
    Am, ok = pref.freeze(N, hits)
    y64, ok64 = pref.project(x, bounds, K, flags=flags, transpose=bool(transpose))
    y_ld, _ = pref.project(x, bounds, K, flags=flags, transpose=bool(transpose), dtype=np.longdouble)
    assert ok.all() and ok64.all()
    f64_term = 4.0 * float(np.abs(y64 - y_ld.astype(np.float64)).max())
    bound = 2.0**-24 * (np.abs(x.astype(np.float64) - y64) + np.abs(y64)) + f64_term
    assert f64_term <= 1e-10

    def check(o):
        ratio = float((np.abs(o["x"].astype(np.float64) - y64) / bound).max())
        assert ratio <= 1.0, ratio
        assert np.abs(o["a"]).min() > 0

    def call(c, v, ld):
        out, a = subscans.project(v.x, bounds, v.A, v.ok, flags=v.flags, transpose=bool(transpose), coefficients=True, ctx=c)
        assert out is v.x
        return dict(a=a)

    return Case(dict(x=IO(x, "ld_x"), flags=I(flags, "ld_f"), A=I(Am), ok=I(ok)), call, check)


def line_normal(ctx):
    import lines_ref
    from test_host_lines import generic_nu, make_bounds, rows, sum_bounds

    from maria_amd import lines

    L, n_poly, T = 2, 1, T0
    x, model, flags = rows(D, T, 35, False)
    bounds = make_bounds(T, 35)
    nu = generic_nu(D, L, 35)
    N_ref, r_ref, h_ref, aN, ar, dN, dr = lines_ref.normal_equations(x, bounds, nu, n_poly, flags=flags, model=model)
    bN, br = sum_bounds(bounds, aN, ar, dN, dr)

    def check(o):
        exact(o["hits"], h_ref)
        assert np.all(np.abs(o["N"] - N_ref) <= bN) and np.all(np.abs(o["r"] - r_ref) <= br)

    def call(c, v, ld):
        N, r, hits = lines.normal_equations(v.x, bounds, nu, n_poly=n_poly, flags=v.flags, model=v.model, ctx=c)
        return dict(N=N, r=r, hits=hits)

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f")), call, check)


def line_apply(ctx):
    import lines_ref
    from test_host_lines import make_bounds, quarter_nu

    from maria_amd import lines

    L, n_poly, T, sign = 2, 1, T0, -1
    K = n_poly + 2 * L
    rng = np.random.default_rng(36)
    x = rng.integers(-64, 65, (D, T)).astype(np.float32)
    bounds = make_bounds(T, 36)
    S = len(bounds) - 1
    nu = quarter_nu(D, L)  # carriers of exactly 0 and +-1: bit for bit
    a = rng.integers(-64, 65, (D, S, K)) / 8.0
    want = lines_ref.apply(x, bounds, nu, a, n_poly, sign=sign)

    def call(c, v, ld):
        assert lines.apply(v.x, bounds, nu, v.a, n_poly, sign=sign, out=v.y, ctx=c) is v.y

    return Case(dict(x=I(x, "ld_x"), a=I(a), y=O((D, T), np.float32, "ld_y")), call, lambda o: exact(o["y"], want))


def segment_moments(ctx):
    import cuts_ref
    from test_gpu_subscans import make_bounds, rows

    from maria_amd import cuts

    T = T0
    x, model, flags = rows(D, T, 37, exact=False)
    bounds = make_bounds(T, 37)
    flags[D - 1, bounds[2]:bounds[3]] = 2
    want = cuts_ref.moments(x, bounds, flags=flags, model=model)

    def check(o):
        for k in ("hits", "pairs", "min", "max"):
            assert np.array_equal(o[k], want[k]), k
        for k, b in cuts_ref.bounds_of(want).items():
            assert np.all(np.abs(o[k] - want[k]) <= b), k

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f")),
                lambda c, v, ld: cuts.moments(v.x, bounds, flags=v.flags, model=v.model, ctx=c)._asdict(), check)


def segment_flag(ctx):
    import cuts_ref
    from test_gpu_resident_trips import FLAG_TILE
    from test_gpu_subscans import make_bounds

    from maria_amd import cuts

    T, value = 2 * FLAG_TILE + 517, 2
    rng = np.random.default_rng(38)
    bounds = make_bounds(T, 1)
    S = len(bounds) - 1
    old = ((rng.random((D, T)) < 0.1) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    mask = (rng.random((D, S)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (D, S)).astype(np.uint8)
    mask[:, np.argmax(np.diff(bounds))] = 1  # the longest segment in every row
    want = cuts_ref.flag_segments(old, bounds, mask, value)
    assert all((want[d] != old[d]).any() for d in range(D))
    def call(c, v, ld):
        assert cuts.flag_segments(v.flags, bounds, v.mask, value, ctx=c) is v.flags

    return Case(dict(flags=IO(old, "ld_f"), mask=I(mask)), call, lambda o: exact(o["flags"], want))


def gram(ctx):
    import covariance_ref

    from maria_amd import covariance

    block = getattr(covariance, "GRAM_BLOCK", 256)
    T = 2 * block + 3
    rng = np.random.default_rng(39)
    x = rng.integers(-16, 17, (D, T)).astype(np.float32)  # integers: every float32 block sum and the float64 total exact
    model = rng.integers(-4, 5, (D, T)).astype(np.float32)
    flags = ((rng.random((D, T)) < 0.1) * rng.integers(1, 3, (D, T))).astype(np.uint8)
    center = np.array([1.0, -2.0, 0.0])
    want = covariance_ref.gram_exact_int(covariance_ref.z_of(x, model, flags, center), ORDER)
    n_want = covariance_ref.counts(flags, D, T, ORDER)

    def check(o):
        assert np.array_equal(o["G"], want.astype(np.float64))
        exact(o["n"], n_want)

    def call(c, v, ld):
        G, n = covariance.gram(v.x, center=v.center, rows=ORDER, flags=v.flags, model=v.model, ctx=c)
        return dict(G=G, n=n)

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f"), center=I(center)), call, check)


# ---- beam fit ----

@functools.lru_cache(maxsize=None)
def _beam_case():
    """beamfit_ref.make_case's daisy scan over a moving source in the sky frame, without its last detector (which is
    parked five degrees off and never nears the source): all three rows cross it."""
    import beamfit_ref as R

    case = R.make_case("ra/dec", drift=True, K=5, D=D + 1, T=R.T_CASE)
    assert case["T"] == T0
    return {k: (v[:D] if k in ("nominal", "truth", "x", "model", "dist2") else D if k == "D" else v) for k, v in case.items()}


def _pointing(case, with_offsets):
    p = dict(az=on_device(case["az"]), el=on_device(case["el"]), transform=on_device(np.ascontiguousarray(case["transform"].reshape(-1, 9))))
    if with_offsets:
        p["dx"], p["dy"] = on_device(case["nominal"][:, 0].astype(np.float32)), on_device(case["nominal"][:, 1].astype(np.float32))
    return p


def source_flag(ctx):
    import beamfit_ref as R
    from test_gpu_beamfit import MARGIN

    from maria_amd import beamfit

    case = _beam_case()
    T, value = case["T"], 5
    dist = np.sqrt(case["dist2"])
    radius = float(np.quantile(dist, 0.5))  # cuts every detector's scan
    before = np.random.default_rng(5).choice(np.array([0, 2, 8, 10], np.uint8), size=(D, T))
    unsure = np.abs(dist - radius) <= MARGIN * R.SPACING
    hit = dist > radius
    want = np.where(hit, before | np.uint8(value), before)
    assert unsure.mean() < 0.01 and all(0.02 < hit[d].mean() < 0.98 for d in range(D))

    def call(c, v, ld):
        beamfit.source_flags(_pointing(case, True), case["center"], radius, src=on_device(case["src"]), inside=False, value=value, flags=v.flags, ctx=c)

    def check(o):
        assert not ((o["flags"] != want) & ~unsure).any()
        assert np.all((o["flags"] == before) | (o["flags"] == (before | np.uint8(value))))

    return Case(dict(flags=IO(before, "ld_f")), call, check)


def beam_normal(ctx):
    import beamfit_ref as R
    from test_gpu_beamfit import MARGIN

    from maria_amd import beamfit

    case = _beam_case()
    flags = R.window_of(case)
    flags[1, ::7] = 4
    params = R.start_of(case)
    model = case["model"]
    x = (case["x"] + model).astype(np.float32)
    hits, chi2, JtJ, Jtr = R.sums(x, case["G"], params, flags, model, case["src"])
    env = R.envelope(x, case["G"], params, flags, model, case["src"])
    assert hits.min() > 100

    def call(c, v, ld):
        n = beamfit.normal_equations(v.x, _pointing(case, False), case["center"], on_device(params), flags=v.flags, model=v.model,
                                     src=on_device(case["src"]), ctx=c)
        return dict(hits=n.hits, chi2=n.chi2, JtJ=n.JtJ, Jtr=n.Jtr)

    def check(o):
        exact(o["hits"], hits)
        live = hits > 0
        for name, want, e in zip(("chi2", "JtJ", "Jtr"), (chi2, JtJ, Jtr), env):
            g = o[name]
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(e[live] > 0, np.abs(g[live] - want[live]) / e[live], np.where(g[live] == want[live], 0.0, np.inf))
            assert ratio.max() <= MARGIN, (name, float(ratio.max()))
            assert np.all(g[~live] == 0)

    return Case(dict(x=I(x, "ld_x"), model=I(model, "ld_m"), flags=I(flags, "ld_f")), call, check)


# ---- time constants, HWP ----

def _poles():
    import timeconst_ref

    x, _ = timeconst_ref.case(D, T0)
    return x, np.array([timeconst_ref.POLES[-1], 0.5, 0.78])


def _onepole(in_place):
    import timeconst_ref

    from maria_amd import time_constants

    x, a = _poles()
    y64 = timeconst_ref.forward64(x, a, 1)
    bound = timeconst_ref.forward_bound(y64, x, a)

    def check(o):
        assert np.all(np.abs(o["x" if in_place else "y"].astype(np.float64) - y64) <= bound)

    if in_place:
        return Case(dict(x=IO(x, "ld_x+ld_y"), a=I(a)), lambda c, v, ld: nothing(time_constants.apply(v.x, v.a, "steady", out=v.x, ctx=c)), check)
    return Case(dict(x=I(x, "ld_x"), a=I(a), y=O((D, T0), np.float32, "ld_y")),
                lambda c, v, ld: nothing(time_constants.apply(v.x, v.a, "steady", out=v.y, ctx=c)), check)


def _onepole_inverse(in_place):
    import timeconst_ref

    from maria_amd import time_constants

    y, a = _poles()
    want = timeconst_ref.inverse(y, a, 1)
    if in_place:
        return Case(dict(y=IO(y, "ld_y+ld_x"), a=I(a)), lambda c, v, ld: nothing(time_constants.deconvolve(v.y, v.a, "steady", out=v.y, ctx=c)),
                    lambda o: exact(o["y"], want))
    return Case(dict(y=I(y, "ld_y"), a=I(a), x=O((D, T0), np.float32, "ld_x")),
                lambda c, v, ld: nothing(time_constants.deconvolve(v.y, v.a, "steady", out=v.x, ctx=c)), lambda o: exact(o["x"], want))


def demodulate(ctx):
    from test_gpu_resident_trips import demodulate_case

    from maria_amd import downsample, hwp

    q, n_taps = 3, 41
    T_out = 2 * hwp.TILE_OUTPUTS + 37
    T = q * T_out - 1
    assert downsample.output_length(T, q) == T_out
    x, carrier, ht, hp, want, tols = demodulate_case(D, T, q, n_taps)

    def check(o):
        for k, name in enumerate("tqu"):
            worst = float((np.abs(o[name].astype(np.float64) - want[k]) / tols[k]).max())
            assert worst <= 1.0, (name, worst)

    outs = {name: O((D, T_out), np.float32, "ld_y") for name in "tqu"}
    return Case(dict(x=I(x, "ld_x"), carrier=I(carrier), ht=I(ht), hp=I(hp), **outs),
                lambda c, v, ld: c.call("mrx_tod_demodulate", P(v.x), ld.ld_x, D, T, q, P(v.carrier), P(v.ht), P(v.hp), n_taps, P(v.t), P(v.q), P(v.u),
                                        ld.ld_y), check)


def hwp_modulate(ctx):
    from test_gpu_resident_trips import T3, modulate_case

    from maria_amd import hwp

    si, sc, ss, carrier, want, tol = modulate_case(D)
    return Case(dict(i=I(si, "ld_in"), c=I(sc, "ld_in"), s=I(ss, "ld_in"), carrier=I(carrier), out=O((D, T3), np.float32, "ld_out")),
                lambda c, v, ld: nothing(hwp.modulate(v.i, v.c, v.s, v.carrier, out=v.out, ctx=c)),
                lambda o: exact(np.abs(o["out"].astype(np.float64) - want) <= tol, np.ones((D, T3), bool)))


# ---- pre-processing, K_RJ ----

def detrend_window(ctx):
    import scipy.signal
    from test_gpu_todproc_kernels import _rows, _ulp_check

    T = T0
    x = _rows(D, T, seed=41)
    w = scipy.signal.windows.hann(T)
    ref = x.copy()
    ref -= np.linspace(ref[:, 0], ref[:, -1], T).T
    ref *= w
    return Case(dict(x=IO(x, "ld"), window=I(w), work=O((2 * D,), np.float64)),
                lambda c, v, ld: c.call("mrx_tod_detrend_window", P(v.x), ld.ld, D, T, 1, P(v.window), P(v.work)),
                lambda o: _ulp_check(o["x"], ref))


def detrend_window_transpose(ctx):
    import filter_aware_ref
    import scipy.signal
    from test_gpu_filter_aware import STEP_TOL
    from test_gpu_todproc_kernels import _rows, _worst_row

    T = T0
    y = _rows(D, T, seed=42)
    w = scipy.signal.windows.tukey(T, alpha=0.5)
    want = filter_aware_ref.slope_transpose(y.astype(np.float64) * w)
    return Case(dict(x=IO(y, "ld"), window=I(w)),
                lambda c, v, ld: c.call("mrx_tod_detrend_window_transpose", P(v.x), ld.ld, D, T, 1, P(v.window)),
                lambda o: _worst_row(o["x"], want, STEP_TOL))


def _sosfilt(ctx, transpose):
    import test_gpu_todproc_kernels as k
    from test_gpu_filter_aware import STEP_TOL, _ref_sosfilt_transpose

    from maria_amd import tod_processing as tp

    chunk = ctx.lib.mrx_sosfilt_chunk()
    T = 3 * chunk + 37  # three chunks and a remainder
    sos = k._cascade((("low", 1), ("high", 1)))
    M = tp.chunk_matrix(sos, chunk)
    x = k._rows(D, T, seed=43 + transpose)
    want = _ref_sosfilt_transpose(sos, x, 1) if transpose else k._ref_sosfilt(sos, x, 1)
    need = C.c_size_t()
    assert ctx.lib.mrx_sosfilt_work_doubles(D, T, len(sos), C.byref(need)) == 0
    entry = "mrx_sosfilt_transpose" if transpose else "mrx_sosfilt"

    def call(c, v, ld):
        rc = getattr(c.lib, entry)(c.handle, sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos), P(v.M), P(v.x), ld.ld_in, D, T, 1, P(v.y), ld.ld_out,
                                   P(v.work))
        assert rc == 0, rc

    return Case(dict(x=I(x, "ld_in"), M=I(M), y=O((D, T), np.float32, "ld_out"), work=O((need.value,), np.float64)), call,
                lambda o: k._worst_row(o["y"], want, STEP_TOL) if transpose else k._worst_row(o["y"], want))


def _krj(entry):
    from test_gpu_calibration import _cal_tables

    from maria_amd import pipeline_host
    from oracle import hotpath

    T = T0
    rng = np.random.default_rng(44)
    tables, polarized = _cal_tables(2), [True, False]
    axis, dens = pipeline_host.collapse_calibration(tables, 280.0, 2.5, polarized)
    bore_el = np.radians(55.0 + 3.0 * np.sin(np.linspace(0.0, 9.0, T))).astype(np.float32)
    offsets = np.radians(rng.uniform(-0.5, 0.5, (D, 2)))
    band = np.array([0, 1, 0], np.int32)
    scale = rng.uniform(0.8, 1.2, D).astype(np.float32)
    x = rows3(T, 45, 1.0, 20.0)
    _, el_det = hotpath.broadcast(offsets, np.zeros(T), bore_el)
    # detector d (its offsets, band and scale) owns row ORDER[d]
    per_pw = hotpath.calibrate_to_krj(np.ones((D, T), np.float32), band, tables, 280.0, 2.5, el_det, polarized).astype(np.float64)
    factor = scale[:, None].astype(np.float64) * (per_pw if entry == "mrx_tod_to_krj" else 1.0 / per_pw)
    want = np.empty((D, T))
    want[ORDER] = x[ORDER].astype(np.float64) * factor

    def check(o):
        from helpers import rel_err

        assert rel_err(o["x"], want) <= 1e-5  # tests/test_gpu_calibration.py: the oracle's bound

    return Case(dict(x=IO(x, "ld"), scale=I(scale), rows=I(ORDER), bore_el=I(bore_el), dx=I(offsets[:, 0].astype(np.float32)),
                     dy=I(offsets[:, 1].astype(np.float32)), band=I(band), axis=I(axis.astype(np.float32)), values=I(dens)),
                lambda c, v, ld: c.call(entry, P(v.x), ld.ld, D, T, P(v.scale), P(v.rows), P(v.bore_el), P(v.dx), P(v.dy), P(v.band), P(v.axis),
                                        P(v.values), len(axis), len(dens)), check)


# ---- mappers ----

@functools.lru_cache(maxsize=None)
def _map_problem():
    from test_gpu_mlmap import Problem

    return Problem(D=D, T=T0, n=(12, 16), S=1, frame="sky", gamma=np.zeros(D))  # Stokes weight 0.5: a power of two


def _grain(seed):
    """(tod, weight) on a power-of-two grain: every product and every float64 sum of them is exact in any order."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-64, 65, (D, T0)) / 8.0).astype(np.float32), (rng.integers(1, 5, (D, T0)) / 2.0).astype(np.float32)


def bin_map(ctx):
    from test_gpu_destripe import _kernel_P, _rel

    p = _map_problem()
    tod, weight = _grain(46)
    Pk, _ = _kernel_P(ctx, p)
    W = weight.astype(np.float64).ravel()
    ref_sum = (Pk.T @ (W * tod.astype(np.float64).ravel())).reshape(p.map_shape)
    ref_wgt = (abs(Pk).T @ W).reshape(p.map_shape)
    assert np.count_nonzero(ref_wgt) > 20

    def check(o):
        assert _rel(o["sum"], ref_sum) <= 1e-12 and _rel(o["wgt"], ref_wgt) <= 1e-12

    return Case(dict(tod=I(tod, "ld_tod"), weight=I(weight, "ld_weight"), sum=IO(np.zeros(p.map_shape)), wgt=IO(np.zeros(p.map_shape))),
                lambda c, v, ld: c.call("mrx_bin_map", C.byref(p.sky()), P(v.tod), ld.ld_tod, P(v.weight), ld.ld_weight, *p.point(), P(v.sum), P(v.wgt)),
                check)


def map_project(ctx):
    from test_gpu_mlmap import _flip_tolerant_close

    p = _map_problem()
    x = p.smooth_map()
    ref = (p.P @ x.ravel()).reshape(p.D, p.T)
    return Case(dict(x=I(x), out=O((D, T0), np.float32, "ld_out", fill=np.nan)),
                lambda c, v, ld: c.call("mrx_map_project", C.byref(p.sky()), P(v.x), *p.point(), 1.0, 0.0, P(v.out), ld.ld_out),
                lambda o: _flip_tolerant_close(o["out"].astype(np.float64), ref, 2e-6, 2e-3))


def baseline_reduce(ctx):
    from test_gpu_destripe import _F, _rel

    p = _map_problem()
    L = 100
    tod, weight = _grain(47)
    F, nb = _F(D, T0, L)
    W = weight.astype(np.float64)
    ref = (F.T @ (W * tod).ravel()).reshape(D, nb)
    ref_h = (F.T @ W.ravel()).reshape(D, nb)

    def check(o):
        assert _rel(o["y"], ref) <= 1e-12 and _rel(o["hits"], ref_h) <= 1e-12

    return Case(dict(tod=I(tod, "ld_tod"), weight=I(weight, "ld_weight"), y=IO(np.zeros((D, nb))), hits=IO(np.zeros((D, nb)))),
                lambda c, v, ld: c.call("mrx_baseline_reduce", C.byref(p.sky()), P(v.tod), ld.ld_tod, None, 1.0, P(v.weight), ld.ld_weight, None, None,
                                        L, *p.point(), P(v.y), P(v.hits)), check)


# ---- the table: entry -> (the variants' builders, the pitched roles of all variants) ----

def only(builder):
    return {"": builder}


TABLE = {
    "mrx_tod_welch": (only(welch), ("ld",)),
    "mrx_tod_noise_filter": (only(noise_filter), ("ld_x", "ld_y", "ld_w")),
    "mrx_tod_noise_filter_modes": (only(noise_filter_modes), ("ld_x", "ld_y", "ld_w")),
    "mrx_tod_mode_project": (only(mode_project), ("ld_x",)),
    "mrx_tod_decimate": (only(decimate), ("ld_x", "ld_y")),
    "mrx_tod_median_residual": (only(median_residual), ("ld_x", "ld_r")),
    "mrx_tod_glitch_flag": (only(glitch_flag), ("ld_x", "ld_f")),
    "mrx_tod_gap_fill": (only(gap_fill), ("ld_x", "ld_f")),
    "mrx_tod_step_stat": (only(step_stat), ("ld_x", "ld_f", "ld_s")),
    "mrx_tod_jump_find": (only(jump_find), ("ld_s", "ld_f")),
    "mrx_tod_jump_height": (only(jump_height), ("ld_x", "ld_f")),
    "mrx_tod_jump_fix": (only(jump_fix), ("ld_x", "ld_y")),
    "mrx_tod_bin_reduce": (only(bin_reduce), ("ld_x", "ld_m", "ld_f")),
    "mrx_tod_bin_apply": (only(bin_apply), ("ld_x", "ld_y")),
    "mrx_tod_column_mean": (only(column_mean), ("ld_x", "ld_m", "ld_f", "ld_c")),
    "mrx_tod_regress_normal": (only(regress_normal), ("ld_x", "ld_m", "ld_f", "ld_b")),
    "mrx_tod_regress_apply": (only(regress_apply), ("ld_x", "ld_b", "ld_y")),
    "mrx_tod_column_fit": (only(column_fit), ("ld_x", "ld_m", "ld_f", "ld_c")),
    "mrx_tod_column_apply": (only(column_apply), ("ld_x", "ld_c", "ld_y")),
    "mrx_tod_segment_normal": (only(segment_normal), ("ld_x", "ld_m", "ld_f")),
    "mrx_tod_segment_apply": (only(segment_apply), ("ld_x", "ld_y")),
    "mrx_tod_segment_project": (only(segment_project), ("ld_x", "ld_f")),
    "mrx_tod_line_normal": (only(line_normal), ("ld_x", "ld_m", "ld_f")),
    "mrx_tod_line_apply": (only(line_apply), ("ld_x", "ld_y")),
    "mrx_tod_segment_moments": (only(segment_moments), ("ld_x", "ld_m", "ld_f")),
    "mrx_tod_segment_flag": (only(segment_flag), ("ld_f",)),
    "mrx_tod_gram": (only(gram), ("ld_x", "ld_m", "ld_f")),
    "mrx_tod_source_flag": (only(source_flag), ("ld_f",)),
    "mrx_tod_beam_normal": (only(beam_normal), ("ld_x", "ld_m", "ld_f")),
    "mrx_tod_onepole": ({"": lambda ctx: _onepole(False), "in place": lambda ctx: _onepole(True)}, ("ld_x", "ld_y", "ld_x+ld_y")),
    "mrx_tod_onepole_inverse": ({"": lambda ctx: _onepole_inverse(False), "in place": lambda ctx: _onepole_inverse(True)},
                                ("ld_y", "ld_x", "ld_y+ld_x")),
    "mrx_tod_demodulate": (only(demodulate), ("ld_x", "ld_y")),
    "mrx_tod_hwp_modulate": (only(hwp_modulate), ("ld_in", "ld_out")),
    "mrx_tod_detrend_window": (only(detrend_window), ("ld",)),
    "mrx_sosfilt": (only(lambda ctx: _sosfilt(ctx, False)), ("ld_in", "ld_out")),
    "mrx_tod_detrend_window_transpose": (only(detrend_window_transpose), ("ld",)),
    "mrx_sosfilt_transpose": (only(lambda ctx: _sosfilt(ctx, True)), ("ld_in", "ld_out")),
    "mrx_tod_to_krj": (only(lambda ctx: _krj("mrx_tod_to_krj")), ("ld",)),
    "mrx_tod_from_krj": (only(lambda ctx: _krj("mrx_tod_from_krj")), ("ld",)),
    "mrx_bin_map": (only(bin_map), ("ld_tod", "ld_weight")),
    "mrx_map_project": (only(map_project), ("ld_out",)),
    "mrx_baseline_reduce": (only(baseline_reduce), ("ld_tod", "ld_weight")),
}


def table_roles(entry):
    """The pitch arguments an entry's roles cover: what tests/test_host_wide_rows.py holds against the header."""
    return sorted({token for role in TABLE[entry][1] for token in role.split("+")})


CASES, BASE = {}, {}


def built(ctx, entry, variant):
    """(the case of a variant of the entry, its outputs on contiguous arrays): built, run and held to the reference once."""
    key = (entry, variant)
    if key not in CASES:
        CASES[key] = TABLE[entry][0][variant](ctx)
        out, intact, unchanged = run(ctx, CASES[key])
        assert intact and unchanged, "the contiguous call changed an input"
        CASES[key].check(out)
        BASE[key] = out
    return CASES[key], BASE[key]


def case_of(ctx, entry, role):
    """The variant of the entry that has the role."""
    for variant in TABLE[entry][0]:
        case, base = built(ctx, entry, variant)
        if role in case.roles():
            return case, base
    raise AssertionError(f"{entry} has no variant with the role {role}")


PARAMS = [(entry, role) for entry, (_, roles) in TABLE.items() for role in roles]
IDS = [f"{entry}-{role}" for entry, role in PARAMS]


@pytest.fixture(scope="module")
def arena(gpu_ctx):
    import torch

    torch.cuda.reset_peak_memory_stats()
    started = time.perf_counter()
    a = wr.Arena(T_MAX, DEV)
    yield a
    torch.cuda.synchronize()
    print(f"\nwide rows: {time.perf_counter() - started:.1f} s from the arena's allocation, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB (arena {a.bytes / 2**30:.2f} GiB)")
    a.release()


@pytest.mark.parametrize("entry", list(TABLE))
def test_the_roles_of_the_table_are_the_cases(gpu_ctx, entry):
    """The roles the table declares are the pitch arguments of the entry's cases, and the contiguous call meets the
    reference."""
    got = set()
    for variant in TABLE[entry][0]:
        got |= set(built(gpu_ctx, entry, variant)[0].roles())
    assert got == set(TABLE[entry][1])


@pytest.mark.parametrize("layout", wr.LAYOUTS)
@pytest.mark.parametrize("entry,role", PARAMS, ids=IDS)
def test_wide_rows(gpu_ctx, arena, entry, role, layout):
    case, base = case_of(gpu_ctx, entry, role)
    out, intact, unchanged = run(gpu_ctx, case, arena, role, layout)
    assert not differing(out, base), f"{differing(out, base)} differ from the contiguous call"
    case.check(out)
    assert intact, "written outside the rows"
    assert unchanged, "an input changed"


@pytest.mark.parametrize("entry,role", PARAMS, ids=IDS)
def test_a_wrong_pitch_is_noticed(gpu_ctx, arena, entry, role):
    """The compact pitch for the wide array: rows 1 and 2 are read or written in the arena's head, and the comparison with
    the contiguous call or the guard strips must say so."""
    case, base = case_of(gpu_ctx, entry, role)
    out, intact, unchanged = run(gpu_ctx, case, arena, role, "aligned", wrong=True)
    assert differing(out, base) or not intact or not unchanged, "a misplaced row went unnoticed: the case is too weak"
