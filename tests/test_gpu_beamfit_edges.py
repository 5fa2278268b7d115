"""The beam fit's two kernels (mrx_tod_source_flag, mrx_tod_beam_normal) off the field centre and at the
edges of their loops, against tests/beamfit_ref.py under test_gpu_beamfit.py's acceptance: hits equal, and
chi2, JtJ and Jtr within MARGIN = 4 of ``beamfit_ref.envelope``.

B  off-axis geometry: the frame's centre 0.1 rad and more from the scan (the asinf branch of the asin(r)/r factor on kept
   samples) and the array at a common offset (the curvature term h of dc/d(dx, dy), its series and its far branch).
   tests/test_host_beamfit.py shows on the CPU that a Jacobian wrong in either term misses these cases by more than
   2 MARGIN envelopes in every row.
C  shapes at the seams of a wave's 256 samples, a thread's four, the 16-row group and the 16-tile chunk, over a source the
   boresight never leaves, so that every sample counts; with and without flags, NaN under every flag and in the padding.
D  one kept sample a row, at every seam: identities that hold in every bit only if nothing else was added.
E  one call on all rows against D calls on one row each, bit for bit.
F  what the C entries refuse, and a work buffer of exactly the size they ask for."""

import numpy as np
import pytest
from test_gpu_beamfit import DEV, MARGIN, pointing_of, run_normal
from test_gpu_jumps import device_rows, untouched_outside

import beamfit_ref as R

pytestmark = pytest.mark.gpu
HOVER = {}
NAMES = ("chi2", "JtJ", "Jtr")


def hover_of(frame, K, D, T):
    """The shared hover cases, made once and never changed."""
    key = (frame, K, D, T)
    if key not in HOVER:
        HOVER[key] = R.make_hover_case(frame, K, D, T)
    return HOVER[key]


def numpy_of(n):
    return n.hits.cpu().numpy(), (n.chi2.cpu().numpy(), n.JtJ.cpu().numpy(), n.Jtr.cpu().numpy())


def accept(label, n, reference, env):
    """The acceptance of test_beam_normal_against_reference: hits equal, rows without hits all zero, the others within
    MARGIN envelopes; prints the largest ratio of each sum (DESIGN 3.31 records them)."""
    hits, got = numpy_of(n)
    assert np.array_equal(hits, reference[0]), label
    assert np.array_equal(got[1], np.swapaxes(got[1], 1, 2)), label
    live = reference[0] > 0
    worst = []
    for name, g, want, e in zip(NAMES, got, reference[1:], env):
        assert np.all(g[~live] == 0), (label, name)
        diff = np.abs(g[live] - want[live])
        ratio = np.where(e[live] > 0, diff / np.where(e[live] > 0, e[live], 1.0), np.where(diff == 0, 0.0, np.inf))
        worst.append(float(ratio.max()) if live.any() else 0.0)
    print(f"{label}: largest |kernel - reference| / envelope: chi2 {worst[0]:.3e}, JtJ {worst[1]:.3e}, Jtr {worst[2]:.3e}")
    for name, w in zip(NAMES, worst):
        assert w <= MARGIN, (label, name, w)


def same_bits(a, b):
    import torch

    return all(torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q)
               for p, q in zip(a, b))


class Padded:
    """A case's inputs in padded device buffers and ``beamfit.normal_equations`` on them.  Without flags the padding of x
    and of the model is 7 and -7; with flags x and the model hold NaN under every flagged sample and in the padding."""

    def __init__(self, gpu_ctx, case, params, flags, with_model, layout):
        import torch

        self.ctx, self.case = gpu_ctx, case
        nan = np.float32("nan")
        model = case["model"] if with_model else None
        x = case["x"] if model is None else (case["x"] + model).astype(np.float32)
        self.reference_inputs = (x, case["G"], params, flags, model, case["src"])
        self.poisoned = flags is not None
        if self.poisoned:
            x = np.where(flags != 0, nan, x)
            model = None if model is None else np.where(flags != 0, nan, model)
        self.xbuf, self.x, _ = device_rows(x, layout, nan if self.poisoned else 7.0)
        self.mbuf = self.model = self.fbuf = self.flags = None
        if model is not None:
            self.mbuf, self.model, _ = device_rows(model, layout, nan if self.poisoned else -7.0)
        if flags is not None:
            self.fbuf, self.flags, _ = device_rows(flags, layout, 3)
        self.par = torch.as_tensor(params).to(DEV)
        self.pointing = pointing_of(case, with_offsets=False)
        self.src = None if case["src"] is None else torch.as_tensor(case["src"]).to(DEV)
        self.inputs = [b for b in (self.xbuf, self.mbuf, self.fbuf, self.par) if b is not None]
        self.before = [b.clone() for b in self.inputs]

    def normal(self, rows=slice(None)):
        import torch

        from maria_amd import beamfit

        n = beamfit.normal_equations(self.x[rows], self.pointing, self.case["center"], self.par[rows], flags=None if self.flags is None else self.flags[rows],
                                     model=None if self.model is None else self.model[rows], src=self.src, ctx=self.ctx)
        torch.cuda.synchronize()
        return n

    def reference(self):
        """(sums, envelope) of the reference, over the columns in which any row keeps a sample (the others add nothing)."""
        x, G, params, flags, model, src = self.reference_inputs
        if flags is not None:
            cols = np.flatnonzero((flags == 0).any(axis=0))
            x, G, flags, model, src = x[:, cols], G[cols], flags[:, cols], None if model is None else model[:, cols], None if src is None else src[cols]
        return R.sums(x, G, params, flags, model, src), R.envelope(x, G, params, flags, model, src)

    def assert_inputs_untouched(self):
        """Every bit of every input buffer, padding included, is what it was; and (this fills the views: call it last)
        nothing outside the views holds anything but the padding's value."""
        assert same_bits(self.inputs, self.before), "an input buffer changed"
        if not self.poisoned:  # (a NaN padding compares unequal to itself: the comparison of the bits above covers it)
            assert untouched_outside(self.xbuf, self.x, 7.0)
            assert self.mbuf is None or untouched_outside(self.mbuf, self.model, -7.0)
        assert self.fbuf is None or untouched_outside(self.fbuf, self.flags, 3)


# ---- B: off the field centre ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("number", sorted(R.OFFAXIS))
def test_beam_normal_off_axis(gpu_ctx, number):
    """The six geometries of DESIGN 3.31 (the host asserts first which branches their samples take) under the acceptance of
    test_beam_normal_against_reference; row 3 is flagged end to end and gives zeros."""
    case, flags, params = R.offaxis_case(number)
    print(R.offaxis_geometry(number))
    spec = R.OFFAXIS[number]
    model = case["model"] if spec["with_model"] else None
    x_ref = case["x"] if model is None else (case["x"] + model).astype(np.float32)
    reference = R.sums(x_ref, case["G"], params, flags, model, case["src"])
    env = R.envelope(x_ref, case["G"], params, flags, model, case["src"])
    assert reference[0][3] == 0 and np.delete(reference[0], 3).min() > 100
    n, same, _ = run_normal(gpu_ctx, case, params, flags, model, spec["layout"])
    assert same, "an input changed"
    accept(f"off-axis case {number} K {case['K']} model {spec['with_model']} {spec['layout']}", n, reference, env)


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("number", [1, 6])
def test_source_flag_off_axis(gpu_ctx, number, layout):
    """As test_source_flag_against_reference_distances, with offsets of 0.12 and 0.44 rad from the centre: the kernel's
    verdict is the reference's except within MARGIN float32 spacings of the radius (fewer than 1 % of the samples, checked
    first); the reference distance from the radius of every sample that differs is printed."""
    import torch

    from maria_amd import beamfit

    case, _, _ = R.offaxis_case(number)
    D, T = case["D"], case["T"]
    dist = np.sqrt(case["dist2"])
    before = np.random.default_rng(5).choice(np.array([0, 2, 8, 10], np.uint8), size=(D, T))
    src = torch.as_tensor(case["src"]).to(DEV)
    for radius, inside, value in ((R.RADIUS, True, 1), (0.4 * R.RADIUS, False, 5)):
        unsure = np.abs(dist - radius) <= MARGIN * R.SPACING
        assert unsure.mean() < 0.01
        hit = dist <= radius if inside else dist > radius
        assert 0.02 < hit.mean() < 0.98  # the radius does cut the scan
        want = np.where(hit, before | np.uint8(value), before)
        buf, view, _ = device_rows(before, layout, 64)
        beamfit.source_flags(pointing_of(case), case["center"], radius, src=src, inside=inside, value=value, flags=view, ctx=gpu_ctx)
        torch.cuda.synchronize()
        got = view.cpu().numpy()
        differ = got != want
        off = np.abs(dist - radius)[differ]
        print(f"off-axis case {number} {layout} radius {radius:.3e}: {int(unsure.sum())} samples within {MARGIN * R.SPACING:.2e} rad of the radius, "
              f"{int(differ.sum())} differ, the farthest {off.max() if off.size else 0.0:.3e} rad from it")
        assert not (differ & ~unsure).any()
        assert np.all((got == before) | (got == (before | np.uint8(value))))
        assert untouched_outside(buf, view, 64)


# ---- C: the seams of the shapes ----------------------------------------------------------------------------------------

SHAPES = [(17, T) for T in (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)] + [(D, 1025) for D in (1, 15, 16, 17, 32, 33)] \
    + [(3, T) for T in (16383, 16384, 16385, 32768, 32769)]


def shape_case(i):
    """(frame, K, with_model, layout) going round with the list's index, so that each value meets short and long T."""
    return ("az/el", "ra/dec")[(i // 3) % 2], (5, 7)[i % 2], bool((i // 2) % 2), ("aligned", "odd")[(i // 4 + i) % 2]


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"{D}x{T}" for D, T in SHAPES])
def test_beam_normal_shape_edges(gpu_ctx, i):
    """Every (D, T) twice: without flags (every sample counts) and with seeded flags (runs over 30 % and single flags, NaN
    under each and in the padding of x and of the model)."""
    D, T = SHAPES[i]
    frame, K, with_model, layout = shape_case(i)
    case = hover_of(frame, K, D, T)
    params = R.start_of(case)
    for flags in (None, R.seeded_flags(D, T, seed=1000 + i)):
        run = Padded(gpu_ctx, case, params, flags, with_model, layout)
        reference, env = run.reference()
        assert reference[0].sum() > 0 and (flags is not None or np.all(reference[0] == T))
        n = run.normal()
        accept(f"{D} x {T} {frame} K {K} model {with_model} {layout} {'no flags' if flags is None else 'flagged'}", n, reference, env)
        run.assert_inputs_untouched()


FLAG_SHAPES = SHAPES[:17]


@pytest.mark.parametrize("i", range(len(FLAG_SHAPES)), ids=[f"{D}x{T}" for D, T in FLAG_SHAPES])
def test_source_flag_shape_edges(gpu_ctx, i):
    """The aligned layout (one 4-byte access a thread) and the odd one (bytes) give the same flags, the reference's outside
    the band; earlier bits stay; ``value`` 1, 128 and 255; a radius of 10 rad sets every sample of D x T with ``inside``
    and none without; the padding keeps its sentinel."""
    import torch

    from maria_amd import beamfit

    D, T = FLAG_SHAPES[i]
    frame = shape_case(i)[0]
    case = hover_of(frame, shape_case(i)[1], D, T)
    dist = np.sqrt(case["dist2"])
    before = np.random.default_rng(i).choice(np.array([0, 2, 8, 10], np.uint8), size=(D, T))
    calls = [(0.5 * R.FWHM, True, 1), (0.6 * R.FWHM, False, 128), (0.4 * R.FWHM, True, 255), (10.0, True, (1, 128, 255)[i % 3]), (10.0, False, 1)]
    for radius, inside, value in calls:
        unsure = np.abs(dist - radius) <= MARGIN * R.SPACING
        hit = dist <= radius if inside else dist > radius
        if radius == 10.0:
            assert hit.all() == inside and hit.any() == inside and not unsure.any()
        want = np.where(hit, before | np.uint8(value), before)
        got = {}
        for layout in ("aligned", "odd"):
            buf, view, _ = device_rows(before, layout, 64)
            beamfit.source_flags(pointing_of(case), case["center"], radius, inside=inside, value=value, flags=view, ctx=gpu_ctx)
            torch.cuda.synchronize()
            got[layout] = view.cpu().numpy()
            assert untouched_outside(buf, view, 64), (layout, radius)
        assert np.array_equal(got["aligned"], got["odd"]), radius
        assert not ((got["odd"] != want) & ~unsure).any(), radius
        assert np.all((got["odd"] == before) | (got["odd"] == (before | np.uint8(value)))), radius
    if T >= 255:
        assert 0.1 < (dist <= 0.5 * R.FWHM).mean() < 0.9  # the radii do cut the track


# ---- D: one kept sample a row ------------------------------------------------------------------------------------------

PROBES = {(5, "odd"): 0, (7, "odd"): 7, (5, "aligned"): 14, (7, "aligned"): 3}  # the rotation of the positions over the rows


def probe_run(gpu_ctx, K, layout):
    case = hover_of(("az/el", "ra/dec")[K == 7], K, R.D_PROBE, R.T_PROBE)
    flags, kept = R.probe_flags(PROBES[(K, layout)])
    return Padded(gpu_ctx, case, R.start_of(case), flags, layout == "aligned", layout), kept


@pytest.mark.parametrize("K,layout", sorted(PROBES))
def test_single_kept_sample(gpu_ctx, K, layout):
    """33 x 33797 (three chunks, the last of two tiles) with every sample flagged, NaN under it, except one a row, at lane
    0 and 63, q = 0 and 3, every wave's edge, both chunk seams and the tail; rows 16 .. 30 keep nothing.  Each sum of a
    live row is then one term plus zeros, so in every bit: JtJ[K-1][K-1] = 1, Jtr[K-1]^2 = chi2, and JtJ[i][j] =
    JtJ[i][K-1] JtJ[j][K-1].  A contribution from any other lane, wave, row or chunk breaks one of them."""
    run, kept = probe_run(gpu_ctx, K, layout)
    n = run.normal()
    hits, (chi2, JtJ, Jtr) = numpy_of(n)
    live = kept >= 0
    assert np.array_equal(hits, live.astype(np.int64))
    for name, g in zip(NAMES, (chi2, JtJ, Jtr)):
        assert np.all(g[~live] == 0) and np.isfinite(g).all(), name
    for d in np.flatnonzero(live):
        assert JtJ[d, K - 1, K - 1] == 1.0, d
        assert Jtr[d, K - 1] * Jtr[d, K - 1] == chi2[d] and chi2[d] > 0, (d, kept[d])
        col = JtJ[d, :, K - 1]
        assert np.array_equal(JtJ[d], col[:, None] * col[None, :]), (d, kept[d])
        assert col[0] >= 0.05  # exp(-q / 2) of the hover case
    reference, env = run.reference()
    accept(f"single kept sample K {K} {layout}", n, reference, env)
    run.assert_inputs_untouched()


# ---- E: rows are independent, bit for bit ------------------------------------------------------------------------------

@pytest.mark.parametrize("which,layout", [("probe", "aligned"), ("probe", "odd"), ("flagged", "aligned"), ("flagged", "odd")])
def test_rows_are_independent_bit_for_bit(gpu_ctx, which, layout):
    """One call on all rows equals D calls on one row each (views of the same buffers, the same pointing) in every bit of
    every output, and so does a second identical call: a wave or row that was skipped, or not skipped, because of its group
    mates changed nothing.  (A one-row call reads its flags by bytes where T is odd: the wide read is compared too.)"""
    import torch

    if which == "probe":
        run, _ = probe_run(gpu_ctx, 7, layout)
    else:
        case = hover_of("ra/dec", 5, 33, 1025)
        run = Padded(gpu_ctx, case, R.start_of(case), R.seeded_flags(33, 1025, seed=77), True, layout)
    n = run.normal()
    again = run.normal()
    assert all(torch.equal(a, b) for a, b in zip(n, again)), "a second call gave other bits"
    assert int(n.hits.sum()) > 0
    for d in range(run.case["D"]):
        alone = run.normal(slice(d, d + 1))
        for name, a, b in zip(("hits",) + NAMES, alone, n):
            assert torch.equal(a, b[d:d + 1]), (name, d)
    run.assert_inputs_untouched()


# ---- F: what the C entries refuse --------------------------------------------------------------------------------------

INVALID = -1  # MRX_ERR_INVALID


def unpack(out, K):
    """(chi2, JtJ, Jtr) of the entry's [D][1 + K (K + 1) / 2 + K] output."""
    out = out.cpu().numpy()
    iu = np.triu_indices(K)
    JtJ = np.zeros((out.shape[0], K, K))
    JtJ[:, iu[0], iu[1]] = out[:, 1:1 + iu[0].size]
    JtJ[:, iu[1], iu[0]] = out[:, 1:1 + iu[0].size]
    return out[:, 0], JtJ, out[:, 1 + iu[0].size:]


def test_entries_refuse_invalid_arguments(gpu_ctx):
    """Every refusal of the two C entries, reached through the context itself (the Python wrappers refuse earlier):
    MRX_ERR_INVALID, outputs untouched, and the context still good for a valid call, which here has a work buffer of exactly
    mrx_tod_beam_normal_work_bytes followed by 4096 sentinel bytes that stay."""
    import ctypes as C

    import torch

    from maria_amd._lib import MrxError, ptr

    D, T, K = 5, 1029, 5
    case = hover_of("ra/dec", K, D, T)
    params = R.start_of(case)
    flags_np = R.seeded_flags(D, T, seed=3)
    x = torch.as_tensor((case["x"] + case["model"]).astype(np.float32)).to(DEV)
    model, flags = torch.as_tensor(case["model"]).to(DEV), torch.as_tensor(flags_np).to(DEV)
    point = pointing_of(case)
    par = torch.zeros((D, 7), dtype=torch.float64, device=DEV)  # (room for the refused K = 6 and for K = 7)
    par.view(-1)[:D * K] = torch.as_tensor(params).to(DEV).view(-1)
    need = C.c_size_t()
    assert gpu_ctx.lib.mrx_tod_beam_normal_work_bytes(D, T, K, C.byref(need)) == 0 and need.value % 4 == 0
    assert gpu_ctx.lib.mrx_tod_beam_normal_work_bytes(D, T, 6, C.byref(need)) == INVALID
    assert gpu_ctx.lib.mrx_tod_beam_normal_work_bytes(0, T, K, C.byref(need)) == INVALID
    assert gpu_ctx.lib.mrx_tod_beam_normal_work_bytes(D, 0, K, C.byref(need)) == INVALID
    need = need.value
    work = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    assert work.data_ptr() % 8 == 0
    nv = 1 + K * (K + 1) // 2 + K
    out = torch.full((D * 36,), -777.0, dtype=torch.float64, device=DEV)  # (K = 7 would write 35 a row: room for it)
    count = torch.full((D,), -7, dtype=torch.int32, device=DEV)
    phi, theta = case["center"]
    nan, inf = float("nan"), float("inf")

    def normal(**over):
        a = dict(ld_x=T, ld_m=T, ld_f=T, T=T, D=D, phi=phi, theta=theta, K=K, work=work.data_ptr(), work_bytes=need)
        a.update(over)
        gpu_ctx.call("mrx_tod_beam_normal", ptr(x), a["ld_x"], ptr(model), a["ld_m"], ptr(flags), a["ld_f"], ptr(point["az"]), ptr(point["el"]), a["T"],
                     ptr(point["transform"]), None, None, a["D"], a["phi"], a["theta"], None, ptr(par), a["K"], ptr(out), ptr(count),
                     C.c_void_p(a["work"]), a["work_bytes"])
        torch.cuda.synchronize()

    refused = [dict(K=6), dict(ld_x=T - 1), dict(ld_m=T - 1), dict(ld_f=T - 1), dict(work_bytes=need - 8), dict(work=work.data_ptr() + 4), dict(D=0),
               dict(T=0), dict(phi=nan), dict(theta=nan), dict(phi=inf)]
    for over in refused:
        with pytest.raises(MrxError) as e:
            normal(**over)
        assert e.value.code == INVALID, over
        assert bool((out == -777.0).all()) and bool((count == -7).all()) and bool((work == 0xA5).all()), over
    normal()
    assert bool((work[need:] == 0xA5).all()), "the entry wrote past the work size it asked for"
    assert bool((out[D * nv:] == -777.0).all())
    x_ref = (case["x"] + case["model"]).astype(np.float32)
    reference = R.sums(x_ref, case["G"], params, flags_np, case["model"], None)
    env = R.envelope(x_ref, case["G"], params, flags_np, case["model"], None)
    assert np.array_equal(count.cpu().numpy(), reference[0]) and reference[0].min() > 100
    for name, g, want, e in zip(NAMES, unpack(out[:D * nv].view(D, nv), K), reference[1:], env):
        assert np.all(np.abs(g - want) <= MARGIN * e), name

    before = np.random.default_rng(1).choice(np.array([0, 2, 8, 10], np.uint8), size=(D, T))
    fl = torch.as_tensor(before).to(DEV)
    radius = 0.5 * R.FWHM

    def source(**over):
        a = dict(T=T, D=D, phi=phi, theta=theta, radius=radius, inside=1, value=4, ld_f=T)
        a.update(over)
        gpu_ctx.call("mrx_tod_source_flag", ptr(point["az"]), ptr(point["el"]), a["T"], ptr(point["transform"]), ptr(point["dx"]), ptr(point["dy"]),
                     a["D"], a["phi"], a["theta"], None, a["radius"], a["inside"], a["value"], ptr(fl), a["ld_f"])
        torch.cuda.synchronize()

    refused = [dict(ld_f=T - 1), dict(D=0), dict(T=0), dict(value=0), dict(value=256), dict(inside=2), dict(radius=-1.0), dict(radius=nan),
               dict(radius=inf), dict(phi=nan), dict(theta=nan)]
    for over in refused:
        with pytest.raises(MrxError) as e:
            source(**over)
        assert e.value.code == INVALID, over
        assert np.array_equal(fl.cpu().numpy(), before), over
    source()
    dist = np.sqrt(case["dist2"])
    unsure = np.abs(dist - radius) <= MARGIN * R.SPACING
    want = np.where(dist <= radius, before | np.uint8(4), before)
    assert not ((fl.cpu().numpy() != want) & ~unsure).any() and 0.1 < (dist <= radius).mean() < 0.9
