"""GPU tests of the noise generator draw for draw: mrx_noise_generate against oracle/noise_philox.py, the
float64 rebuild of the same Philox draws, cells, transform, window mean, interpolation and level.  Unlike the
statistical tests of tests/test_gpu_noise.py, these see a mistake shared by every kernel form or one that keeps
the spectrum roughly right: one wrong cell out of N moves every sample by ~1/sqrt(N) of the row's rms.

Every launch path of noise_generate_impl runs at least once: each period class (N = 4096 with T < 4096; the
radix-16 register first pass at 2^16, 2^17, 2^18; noise_fft64_rows + noise_combine_rows<2, 4, 8, 16> at
2^19 ... 2^22; the 8192-point Stockham first pass at 2^23), the mode-count instances of both first passes, the
MRX_OPT_NOISE_GENERIC forms, one and four lanes with several batches per lane, the epilogue's branches
(scale, loading, accumulation, unaligned rows), the white-only path across its 32 768-row launch split and the
two-rate form at rates 4 and 2 with its kModes instances.

Tolerance: max_t |got - ref| / rms(ref row), per row, below oracle.noise_philox.GPU_BOUND = 7.5e-5, four times the
largest ratio measured on an MI355X.  Measured (largest over each group's rows): one-rate form 1.2e-6 (N = 4096) ...
8.7e-6 (N = 2^23), growing with log2 N as float32 rounding through the transform stages does; two-rate form
3.2e-6 ... 1.3e-5; white-only path 1.9e-5.  The white-only rows are 37 samples long, so their rms is that of 37
normals and the largest of 1.2 M draws sits in the tail, where the hardware logarithm, sine and cosine of
Box-Muller (~1e-6 absolute) weigh most: the largest ratio of all, and still a quarter of the bound.  The float32
budget expected beforehand (rounding through ~log2 N butterfly stages, the hardware sine and cosine, twiddles by
repeated multiplication) was 1e-6 to 1e-5 of the rms: met, the short white rows excepted by a factor of two."""

import contextlib
import ctypes as C

import numpy as np
import pytest

from oracle import noise_philox as onp

pytestmark = pytest.mark.gpu

GENERIC, LANES = 5, 8  # MRX_OPT_NOISE_GENERIC, MRX_OPT_NOISE_LANES


@contextlib.contextmanager
def _options(ctx, opts):
    """Set context options for the block and put back what was there (gpu_ctx is shared by the session)."""
    old = {o: ctx.get_option(o) for o in opts}
    try:
        for o, v in opts.items():
            ctx.set_option(o, v)
        yield
    finally:
        for o, v in old.items():
            ctx.set_option(o, v)


def _period(lib):
    def period(T):
        n1, n2 = C.c_int(), C.c_int()
        assert lib.mrx_noise_period(T, C.byref(n1), C.byref(n2)) == 0
        return n1.value, n2.value

    return period


def _case(ctx, D, T, fs, knee, modes=0, corr=0.4, det_offset=0, seed=7, scale=False, loading=False, accumulate=False,
          layout="packed", work_rows=64, opts=None):
    """Run mrx_noise_generate on one case and rebuild it on the host.  Returns (got, want, base) as float64 arrays;
    base is the TOD accumulated into (or None).  layout: "packed"; "odd_ld" (row stride T + 3); "offset" (rows
    start 4 bytes past a 16-byte boundary)."""
    import torch

    from maria_amd._lib import ptr

    dev = "cuda:0"
    rng = np.random.default_rng(seed + 1000 * modes + D)
    basis = rng.normal(size=(D, modes)) / np.sqrt(max(modes, 1)) if modes else None
    sc = rng.uniform(0.5, 2.0, D) if scale else None
    load = torch.rand((D, T), dtype=torch.float32, device=dev) + 0.5 if loading else None
    per_loading = 0.7 if loading else 0.0
    pad = {"packed": 0, "odd_ld": 3, "offset": 2}[layout]
    buf = torch.as_tensor(rng.normal(size=(D, T + pad)), dtype=torch.float32).to(dev)
    if not accumulate:
        buf.fill_(-7.0)
    out = buf[:, 1 : T + 1] if layout == "offset" else buf[:, :T]
    base = out.cpu().numpy().astype(np.float64) if accumulate else None
    before = buf.clone()
    need = C.c_size_t()
    assert ctx.lib.mrx_noise_work_floats(T, modes, min(work_rows, D), C.byref(need)) == 0
    work = torch.empty(need.value, dtype=torch.float32, device=dev)
    d_basis = None if basis is None else torch.as_tensor(basis, dtype=torch.float32).to(dev)
    d_scale = None if sc is None else torch.as_tensor(sc, dtype=torch.float32).to(dev)
    with _options(ctx, opts or {}):
        ctx.call("mrx_noise_generate", seed, D, det_offset, T, float(fs), float(knee), float(corr), ptr(d_basis), modes,
                 ptr(d_scale), ptr(load), 0 if load is None else load.stride(0), float(per_loading), ptr(out), out.stride(0),
                 int(accumulate), ptr(work), need.value)
        one_rate_only = bool(ctx.get_option(GENERIC) & 8)
    torch.cuda.synchronize()
    # nothing written outside the rows' first T samples
    mask = torch.ones_like(buf, dtype=torch.bool)
    if layout == "offset":
        mask[:, 1 : T + 1] = False
    else:
        mask[:, :T] = False
    assert torch.equal(buf[mask], before[mask])
    got = out.cpu().numpy().astype(np.float64)
    # the reference: basis, scale and loading as the kernel saw them (float32)
    basis32 = None if basis is None else basis.astype(np.float32).astype(np.float64)
    x = onp.generate(seed, D, T, fs, knee, _period(ctx.lib), corr=corr, basis=basis32, det_offset=det_offset,
                     one_rate_only=one_rate_only)
    want = onp.level(x, None if sc is None else sc.astype(np.float32),
                     None if load is None else load.cpu().numpy(), np.float32(per_loading), base)
    return got, want, base


def _check(got, want, base, what):
    r = onp.row_ratios(got, want, base)
    worst = int(np.argmax(r))
    t = int(np.argmax(np.abs(got[worst] - want[worst])))
    print(f"RATIO {what}: {r.max():.3e} (row {worst}, sample {t} of {got.shape[1]})")
    assert np.isfinite(got).all()
    assert r.max() < onp.GPU_BOUND, (what, r.max(), worst, t, np.round(r, 8).tolist()[:16])
    return r.max()


# (id, kwargs of _case): one-rate cases at fs = 50 Hz (knee 2: the two-rate form never applies)
ONE_RATE = [
    # N = 4096 (n2 = 64, n1 = 64): Stockham first pass (kIter 1), register second pass
    ("n4096_modes5_odd_rows_det_offset", dict(D=7, T=3001, modes=5, det_offset=6, scale=True)),
    ("n4096_modes8_generic", dict(D=2, T=4093, modes=8)),
    ("n4096_modes1_one_row", dict(D=1, T=1003, modes=1, det_offset=2)),
    ("n4096_modes0_loading", dict(D=4, T=4095, modes=0, scale=True, loading=True)),
    ("n4096_modes2_lds_pass2_odd_ld", dict(D=5, T=2999, modes=2, scale=True, layout="odd_ld", opts={GENERIC: 1})),
    # N = 2^16 .. 2^18: the radix-16 register first pass (RB 4, 8, 16), its instances 0 .. 5; > 5: Stockham
    ("n65536_modes0_odd_rows", dict(D=5, T=50001, modes=0, det_offset=10)),
    ("n65536_modes3_accumulate", dict(D=4, T=65536, modes=3, accumulate=True)),
    ("n65536_modes6_stockham", dict(D=4, T=40003, modes=6)),
    ("n65536_modes4_lds_pass2_offset", dict(D=3, T=33001, modes=4, scale=True, layout="offset", opts={GENERIC: 1})),
    ("n131072_modes1", dict(D=6, T=100003, modes=1, scale=True)),
    ("n131072_modes5_loading", dict(D=2, T=131071, modes=5, loading=True)),
    ("n131072_modes1_stockham_pass1", dict(D=3, T=70001, modes=1, opts={GENERIC: 2})),
    ("n262144_modes2", dict(D=3, T=200001, modes=2, det_offset=4)),
    ("n262144_modes4_accumulate_odd_ld", dict(D=2, T=262143, modes=4, accumulate=True, layout="odd_ld")),
    ("n262144_modes8_stockham", dict(D=2, T=150001, modes=8)),
    # N = 2^19 .. 2^22: noise_fft64_rows + noise_combine_rows<2, 4, 8, 16>; 2^19 also through the LDS tiles
    ("n2p19_modes5_scale", dict(D=2, T=300001, modes=5, scale=True)),
    ("n2p19_modes2_lds_pass2", dict(D=2, T=400001, modes=2, opts={GENERIC: 1})),
    ("n2p20_modes0_loading_accumulate", dict(D=3, T=600001, modes=0, loading=True, accumulate=True)),
    ("n2p21_modes2_one_row", dict(D=1, T=1500001, modes=2, det_offset=8)),
    ("n2p22_modes1", dict(D=2, T=3000001, modes=1, scale=True)),
    # N = 2^23: the 8192-point Stockham first pass (kIter 16), a single pair
    ("n2p23_modes0", dict(D=2, T=8000001, modes=0)),
    # batching: one lane, a work buffer of three pairs (four batches); four lanes, several batches each,
    # staggered and equal first batches
    ("batches_one_lane", dict(D=21, T=3001, modes=5, scale=True, work_rows=6, opts={LANES: 1})),
    ("batches_four_lanes_staggered", dict(D=600, T=3001, modes=2, det_offset=2, work_rows=512, opts={LANES: 4})),
    ("batches_four_lanes_equal", dict(D=599, T=3001, modes=0, work_rows=512, opts={LANES: 4, GENERIC: 4})),
]


@pytest.mark.parametrize("case", [c[1] for c in ONE_RATE], ids=[c[0] for c in ONE_RATE])
def test_one_rate_form_matches_the_float64_rebuild(gpu_ctx, case):
    got, want, base = _case(gpu_ctx, fs=50.0, knee=2.0, **case)
    _check(got, want, base, str(case))


# fs = 400 Hz: knee 1 -> rate 4, knee 2 -> rate 2 (T >= 32768); the writer's kModes instances 0, 5, 8
TWO_RATE = [
    ("rate4_modes5_loading", dict(D=5, T=40001, knee=1.0, modes=5, det_offset=2, scale=True, loading=True)),
    ("rate2_modes8_accumulate_offset", dict(D=4, T=50003, knee=2.0, modes=8, accumulate=True, layout="offset")),
    ("rate4_modes0_at_the_switch", dict(D=3, T=32768, knee=1.0, modes=0, scale=True)),
    ("rate2_modes2_odd_ld_batches", dict(D=9, T=65537, knee=2.0, modes=2, layout="odd_ld", work_rows=4, opts={LANES: 1})),
    ("one_rate_below_the_switch", dict(D=3, T=32767, knee=1.0, modes=0, scale=True)),
    ("one_rate_forced", dict(D=4, T=40001, knee=1.0, modes=5, scale=True, opts={GENERIC: 8})),
]


@pytest.mark.parametrize("case", [c[1] for c in TWO_RATE], ids=[c[0] for c in TWO_RATE])
def test_two_rate_form_matches_the_float64_rebuild(gpu_ctx, case):
    got, want, base = _case(gpu_ctx, fs=400.0, **case)
    _check(got, want, base, str(case))


@pytest.mark.parametrize("layout,loading", [("packed", False), ("offset", True)])
def test_white_only_path_matches_the_float64_rebuild(gpu_ctx, layout, loading):
    """knee = 0 across the 32 768-row launch split: every row's draws keyed by det_offset + row."""
    got, want, base = _case(gpu_ctx, D=32769, T=37, fs=100.0, knee=0.0, det_offset=4, scale=True, loading=loading,
                            layout=layout)
    _check(got, want, base, f"white {layout} loading={loading}")

