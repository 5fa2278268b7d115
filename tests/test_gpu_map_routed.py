"""The routed map operators (routed_bin in maria_amd/csrc/mrx_map.hip: mrx_bin_map_bucketed, mrx_map_normal_apply,
mrx_bin_map_baselines) at the geometry the project benchmarks: maps of more than 256 and up to 2048 regions, pass-B tile
ranges of several batches of 256 tiles with many segments in a batch, work buffers of several chunks, one tile whose
16 384 contributions all go to one region, both pointing forms, and the 10 000 x 240 000 sample map onto 1024^2.

Every input is a small dyadic rational (TOD k / 8, sample weights {0, 1/4, ..., 4}, Stokes weights {0, +-1/2, +-1},
detector weights {1/2, 1, 2}, maps and baseline amplitudes k / 16), so every float64 partial sum is exact in any order:
the routed form, the atomic form and a float64 reference summed over the kernels' own pixels agree bit for bit.  Each
test proves that premise (the per-pixel sum of |term| stays below 2^(53 - q) for the common denominator 2^-q).  The
pixel of a sample is what mrx_map_project returns for an index map; the pointing itself is tested by test_gpu_map.py.
Bilinear corner weights are not dyadic: there the routed and the atomic forms agree to float64 rounding, and the maps
hold the sums the corners add up to."""

import ctypes as C

import numpy as np
import pytest

from helpers import ROUTED_CASES, routed_geometry, three_chunk_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SW_VALUES = (1.0, 0.5, -0.5, 0.0, -1.0)
W_VALUES = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)
DW_VALUES = (0.5, 1.0, 2.0)
STARE = (7 * 1024, 8 * 1024)  # samples of a boresight stare: tile column 7 (nearest), columns 28-31 (bilinear)


def _pick(values, shape, gen, dtype):
    import torch

    lut = torch.tensor(values, dtype=dtype, device=DEV)
    return lut[torch.randint(0, len(values), shape, generator=gen, device=DEV)]


class Problem:
    """One case's map and TOD on the device: a daisy scan at 400 Hz over a hexagonal focal plane, the map a little
    smaller than the scanned patch (the edge pixels take the rest).  ``stare``: detectors 0-15 packed within a pixel,
    and the boresight fixed at the centre of a region over the samples STARE."""

    def __init__(self, case, seed, weights, fov_deg, S=None, C=None, bilinear=None, stare=False, tod=True):
        import torch

        from maria_amd import synthetic

        c = dict(ROUTED_CASES[case])
        self.case = case
        self.D, self.T, self.n_eta, self.n_xi = c["D"], c["T"], c["n_eta"], c["n_xi"]
        self.S = c["S"] if S is None else S
        self.C = c["C"] if C is None else C
        self.bilinear = c["bilinear"] if bilinear is None else bilinear
        D, T = self.D, self.T
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        t = 1.7e9 + np.arange(T) / 400.0
        self.centre = (float(np.radians(45.0)), float(np.radians(60.0)))
        az, el = synthetic.daisy_scan(t)
        off = synthetic.hex_pack(D, np.radians(fov_deg))
        half = 0.95 * np.radians(0.5 + fov_deg / 2)
        self.eta0, self.deta = half, -2 * half / (self.n_eta - 1)
        self.xi0, self.dxi = -half, 2 * half / (self.n_xi - 1)
        if stare:
            # the centre of the region in the middle of the map
            e = 32 * (-(-self.n_eta // 32) // 2) + 16
            x = 64 * (-(-self.n_xi // 64) // 2) + 32
            a, b = synthetic.offsets_to_phi_theta(self.xi0 + x * self.dxi, self.eta0 + e * self.deta, *self.centre)
            az[STARE[0] : STARE[1]], el[STARE[0] : STARE[1]] = a, b
            off[:16] = synthetic.hex_pack(16, 0.5 * abs(self.dxi))
        f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float32)).to(DEV)  # noqa: E731
        self.az, self.el, self.dx, self.dy = f32(az), f32(el), f32(off[:, 0]), f32(off[:, 1])
        self.sw = _pick(SW_VALUES, (D, self.S), gen, torch.float64)
        self.chan = torch.randint(0, self.C, (D,), generator=gen, device=DEV, dtype=torch.int32)
        self.det_w = _pick(DW_VALUES, (D,), gen, torch.float64)
        self.tod = None
        if tod:
            self.tod = torch.empty((D, T), dtype=torch.float32, device=DEV).random_(-1024, 1025, generator=gen).mul_(0.125)
        self.wts = _pick(W_VALUES, (D, T), gen, torch.float32) if weights else None
        self.gen = gen

    @property
    def n_pix(self):
        return self.n_eta * self.n_xi

    def sky(self, S=None, bilinear=None):
        from maria_amd._lib import MrxSkyMap

        return MrxSkyMap(None, self.C, self.S if S is None else S, self.n_eta, self.n_xi, self.eta0, self.deta, self.xi0, self.dxi,
                         *self.centre, int(self.bilinear if bilinear is None else bilinear), 0)

    def point(self, sw=None):
        """The pointing arguments of every map operator: az, el, T, transform, dx, dy, Stokes weights, channel, D."""
        from maria_amd._lib import ptr

        return (ptr(self.az), ptr(self.el), self.T, None, ptr(self.dx), ptr(self.dy), ptr(self.sw if sw is None else sw),
                ptr(self.chan), self.D)

    def weight_args(self):
        from maria_amd._lib import ptr

        return (ptr(self.wts), 0 if self.wts is None else self.wts.stride(0))

    def geometry(self, entry_bytes, work_bytes=None):
        return routed_geometry(self.C, self.n_eta, self.n_xi, self.D, self.T, self.bilinear, entry_bytes, work_bytes)

    def dyadic_map(self, S, scale=64):
        """A map of integers in [-scale, scale] / 16."""
        import torch

        return torch.empty((S, self.C, self.n_eta, self.n_xi), dtype=torch.float64, device=DEV).random_(-scale, scale + 1, generator=self.gen).div_(16)


def _pixels(ctx, p):
    """c * n_pix + pixel of every sample, as the kernels see it: mrx_map_project of an index map with unit Stokes weights
    (float32 [D, T]; exact below 2^24), in the pointing form the context has selected."""
    import torch

    from maria_amd._lib import ptr

    n = p.C * p.n_pix
    assert n < 1 << 24
    idx = torch.arange(n, dtype=torch.float64, device=DEV).view(1, p.C, p.n_eta, p.n_xi)
    ones = torch.ones((p.D, 1), dtype=torch.float64, device=DEV)
    out = torch.empty((p.D, p.T), dtype=torch.float32, device=DEV)
    ctx.call("mrx_map_project", C.byref(p.sky(S=1, bilinear=False)), ptr(idx), *p.point(sw=ones), 1.0, 0.0, ptr(out), out.stride(0))
    return out


def _scatter(p, pix, n_planes, terms, blk=256):
    """Float64 sums over the samples of each sample's terms at its pixel, and of their magnitudes: two [n_planes, C, n_eta,
    n_xi] tensors.  terms(d0, d1) returns n_planes tensors [d1 - d0, T] (or broadcastable) for detectors [d0, d1)."""
    import torch

    n = p.C * p.n_pix
    acc = torch.zeros((n_planes, n), dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(acc)
    for d0 in range(0, p.D, blk):
        d1 = min(p.D, d0 + blk)
        idx = pix[d0:d1].to(torch.int64)
        for k, v in enumerate(terms(d0, d1, idx)):
            v = v.expand(d1 - d0, p.T).reshape(-1)
            acc[k].index_add_(0, idx.view(-1), v)
            mag[k].index_add_(0, idx.view(-1), v.abs())
        del idx
    shape = (n_planes, p.C, p.n_eta, p.n_xi)
    return acc.view(shape), mag.view(shape)


def _exact(mag, q):
    """The premise of a bit-for-bit comparison: every partial sum is a multiple of 2^-q below 2^(53 - q) in magnitude."""
    assert float(mag.max()) < 2.0 ** (53 - q), (float(mag.max()), q)


def _ref_binning(p, pix):
    """sum = sum W d sw_k, wgt = sum W |sw_k| at each sample's pixel; q = 6 (d / 8, W / 4, sw / 2)."""
    def terms(d0, d1, idx):
        W = p.wts[d0:d1].double() if p.wts is not None else 1.0
        WD = W * p.tod[d0:d1].double()
        sw = p.sw[d0:d1]
        return [WD * sw[:, k : k + 1] for k in range(p.S)] + [W * sw[:, k : k + 1].abs() for k in range(p.S)]

    acc, mag = _scatter(p, pix, 2 * p.S, terms)
    _exact(mag, 6)
    return acc[: p.S], acc[p.S :]


def _max_segments(p, pix, geo):
    """Per chunk, the most non-empty segments any pass-B workgroup lists in one batch: the distinct tiles that hold a
    region's contributions within each batch of 256 tiles of each split's tile range (from the samples' nearest pixels:
    bilinear, a lower bound -- a sample's nearest pixel is one of its corners)."""
    import torch

    out = []
    for ch in geo.chunks:
        present = torch.zeros(geo.R * ch.n_tiles, dtype=torch.bool, device=DEV)
        blk = geo.tile_det * 32
        s = torch.arange(ch.s0, ch.s1, device=DEV)
        for d0 in range(0, p.D, blk):
            d1 = min(p.D, d0 + blk)
            g = pix[d0:d1, ch.s0 : ch.s1].to(torch.int64)
            c, rem = g // p.n_pix, g % p.n_pix
            r = (c * geo.nby + (rem // p.n_xi) // 32) * geo.nbx + (rem % p.n_xi) // 64
            tile = (torch.arange(d0, d1, device=DEV)[:, None] // geo.tile_det) * ch.nc + (s[None, :] - ch.s0) // geo.tile_samples
            present[(r * ch.n_tiles + tile).view(-1)] = True
            del g, c, rem, r, tile
        t = torch.arange(ch.n_tiles, device=DEV)
        split = t // ch.per
        batch = split * ch.batches + (t - split * ch.per) // 256
        counts = torch.zeros((geo.R, ch.sp * ch.batches), dtype=torch.float32, device=DEV)
        counts.index_add_(1, batch, present.view(geo.R, ch.n_tiles).float())
        out.append(int(counts.max()))
    return out


def _report(name, geo, segs):
    per = [ch.per for ch in geo.chunks]
    print(f"\n{name}: R {geo.R} ({geo.regions_per_thread} a thread in pass A), splits {geo.splits}, sp {[ch.sp for ch in geo.chunks]}, "
          f"per {per}, batches {[ch.batches for ch in geo.chunks]}, chunks {len(geo.chunks)} of {[ch.nc for ch in geo.chunks]} columns, "
          f"most segments in a batch {segs}")
    for ch, n in zip(geo.chunks, segs):
        if ch.per > 1:
            assert n > 1, (name, "a batch of one segment")


def _work(nbytes):
    import torch

    return torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)


def _bin(ctx, p, routed, work=None):
    import torch

    from maria_amd._lib import ptr

    out = [torch.zeros((p.S, p.C, p.n_eta, p.n_xi), dtype=torch.float64, device=DEV) for _ in range(2)]
    args = (C.byref(p.sky()), ptr(p.tod), p.tod.stride(0), *p.weight_args(), *p.point(), ptr(out[0]), ptr(out[1]))
    if routed:
        ctx.call("mrx_bin_map_bucketed", *args, ptr(work), work.numel())
    else:
        ctx.call("mrx_bin_map", *args)
    return out


def _equal(a, b, what):
    import torch

    assert torch.equal(a, b), (what, float((a - b).abs().max()), float(b.abs().max()))


@pytest.fixture
def chain(gpu_ctx, request):
    gpu_ctx.set_option(0, request.param)
    yield request.param
    gpu_ctx.set_option(0, 0)


@pytest.fixture(scope="module")
def case_b():
    """Case B's problem: weights, three Stokes planes, two channels, R = 2048."""
    import torch

    p = Problem("B", seed=2, weights=True, fov_deg=0.4)
    yield p
    del p
    torch.cuda.empty_cache()


def _check_binning(ctx, p, name, entry_bytes):
    """The routed binning with the full buffer and with one of three chunks against the atomic form and the reference,
    bit for bit; returns the pixels and the geometry."""
    import torch

    pix = _pixels(ctx, p)
    ref_sum, ref_wgt = _ref_binning(p, pix)
    assert float(ref_wgt.abs().sum()) > 0 and float(ref_sum.abs().max()) > 0
    atomic = _bin(ctx, p, routed=False)
    _equal(atomic[0], ref_sum, "atomic sum")
    _equal(atomic[1], ref_wgt, "atomic weight")
    geo = p.geometry(entry_bytes)
    _report(name, geo, _max_segments(p, pix, geo))
    for wb in (geo.full_bytes, three_chunk_bytes(geo)):
        g = p.geometry(entry_bytes, wb)
        work = _work(wb)
        got = _bin(ctx, p, routed=True, work=work)
        del work
        if len(g.chunks) > 1:
            _report(name + " (chunked)", g, _max_segments(p, pix, g))
        _equal(got[0], ref_sum, f"routed sum, {len(g.chunks)} chunks")
        _equal(got[1], ref_wgt, f"routed weight, {len(g.chunks)} chunks")
    torch.cuda.synchronize()
    return pix, geo, ref_wgt


def test_case_a_nearest_without_weights_and_a_full_tile(gpu_ctx):
    """A: BinMapper's default form (8-byte entries) over 288 regions (two a thread in pass A's scan), pass-B ranges of 54
    tiles; H: one tile whose 16 384 contributions all go to one region (the largest count a word of the table holds)."""
    import torch

    p = Problem("A", seed=1, weights=False, fov_deg=0.5, stare=True)
    pix, geo, _ = _check_binning(gpu_ctx, p, "A", 8)
    assert geo.R == 288 and geo.regions_per_thread == 2 and geo.chunks[0].per > 1
    g = pix[:16, STARE[0] : STARE[1]].to(torch.int64)
    r = (g // p.n_pix * geo.nby + (g % p.n_pix // p.n_xi) // 32) * geo.nbx + (g % p.n_xi) // 64
    assert bool((r == r[0, 0]).all()), "the stare tile's contributions span more than one region"
    print(f"H: tile (0, 7): all {r.numel()} contributions in region {int(r[0, 0])}")
    assert r.numel() == geo.tile_entries


@pytest.mark.parametrize("chain", [0, 1], ids=["composed", "chain"], indirect=True)
def test_case_b_nearest_with_weights_2048_regions(gpu_ctx, case_b, chain):
    """B: 12-byte entries onto 2048 regions (bin_order_kernel's strided loop) with partial regions on both far edges,
    pass-B ranges of 290 tiles (two batches), a last tile row of 8 detectors; I: the same under the float32 pointing
    chain (the other instantiation of every pass A), with the pixels taken under the same option."""
    p = case_b
    pix, geo, wgt = _check_binning(gpu_ctx, p, f"B (chain {chain})", 12)
    assert geo.R == 2048 and geo.chunks[0].per == 290 and geo.chunks[0].batches == 2
    assert p.D % 16 == 8
    assert float(wgt[..., -1, :].abs().sum()) > 0 and float(wgt[..., :, -1].abs().sum()) > 0  # the far edges' partial regions


def _check_bilinear(ref, got, what):
    for g, r in zip(got, ref):
        g, r = g.cpu().numpy(), r.cpu().numpy()
        assert np.abs(r).max() > 0 and np.abs(g - r).max() <= 1e-12 * np.abs(r).max(), what


def test_case_c_bilinear_1081_regions(gpu_ctx):
    """C: bilinear (16-byte entries, tiles of 8 x 256, four corners a sample) onto 1081 regions -- odd and > 1024, so that
    pass A's float2 offsets start at a 4-byte-aligned LDS address -- with pass-B ranges of 493 tiles; routed (full buffer
    and three chunks) against the atomic form, and the sums the corner weights add up to."""
    import torch

    p = Problem("C", seed=3, weights=True, fov_deg=0.4, stare=True)
    pix = _pixels(gpu_ctx, p)
    geo = p.geometry(16)
    _report("C", geo, _max_segments(p, pix, geo))
    assert geo.R == 1081 and geo.chunks[0].per == 493
    # the stare: the tile of detectors 0-7 and samples [7168, 7424) lies inside one region, two pixels from its edges, so
    # that all four corners of every sample do too
    g = pix[:8, STARE[0] : STARE[0] + 256].to(torch.int64)
    e, x = g % p.n_pix // p.n_xi, g % p.n_xi
    assert bool((e // 32 == e[0, 0] // 32).all() and (x // 64 == x[0, 0] // 64).all())
    assert int((e % 32).min()) >= 2 and int((e % 32).max()) <= 29 and int((x % 64).min()) >= 2 and int((x % 64).max()) <= 61
    del pix
    atomic = _bin(gpu_ctx, p, routed=False)
    # the corners of a sample sum to 1 (float64 products of float32 offsets: exact): the weight planes hold sum W |sw_k|,
    # the signal planes sum W d sw_k
    W, d = p.wts.double(), p.tod.double()
    for k in range(p.S):
        sw = p.sw[:, k : k + 1]
        wk = float((W * sw.abs()).sum())
        sk = W * d * sw
        assert abs(float(atomic[1][k].sum()) - wk) <= 1e-12 * wk
        assert abs(float(atomic[0][k].sum()) - float(sk.sum())) <= 1e-12 * float(sk.abs().sum())
    del W, d, sk
    for wb in (geo.full_bytes, three_chunk_bytes(geo)):
        work = _work(wb)
        got = _bin(gpu_ctx, p, routed=True, work=work)
        del work
        _check_bilinear(atomic, got, f"{len(p.geometry(16, wb).chunks)} chunks")
    torch.cuda.synchronize()


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_case_d_one_column_chunks(gpu_ctx, bilinear):
    """D: the sizing functions' minimum buffer -- one column of tiles a chunk, so every chunk edge s0 / s1 -- against the
    full buffer and the atomic form (nearest: and the reference, bit for bit)."""
    p = Problem("D1", seed=4, weights=True, fov_deg=0.4, bilinear=bilinear)
    eb = 16 if bilinear else 12
    full = p.geometry(eb)
    one = p.geometry(eb, full.min_bytes)
    assert one.cols == 1 and len(one.chunks) == full.cols_total > 1
    atomic = _bin(gpu_ctx, p, routed=False)
    if not bilinear:
        ref_sum, ref_wgt = _ref_binning(p, _pixels(gpu_ctx, p))
        _equal(atomic[0], ref_sum, "atomic sum")
        _equal(atomic[1], ref_wgt, "atomic weight")
    for wb in (full.full_bytes, full.min_bytes):
        got = _bin(gpu_ctx, p, routed=True, work=_work(wb))
        if bilinear:
            _check_bilinear(atomic, got, wb)
        else:
            _equal(got[0], atomic[0], wb)
            _equal(got[1], atomic[1], wb)


def _normal(ctx, p, x, work, sw=None, S=None):
    import torch

    from maria_amd._lib import ptr

    y = torch.zeros_like(x)
    ctx.call("mrx_map_normal_apply", C.byref(p.sky(S=S)), ptr(x), *p.weight_args(), ptr(p.det_w), *p.point(sw), ptr(y), ptr(work),
             0 if work is None else work.numel())
    return y


def _ref_normal(p, pix, x, sw=None):
    """P^T W P x at each sample's pixel: sw_k W w_d (P x)_s, (P x)_s = sum_l sw_l x_l; q = 1 + 2 + 1 + 5."""
    sw = p.sw if sw is None else sw
    S = sw.shape[1]
    xf = x.view(S, -1)

    def terms(d0, d1, idx):
        px = sum(sw[d0:d1, l : l + 1] * xf[l][idx] for l in range(S))
        W = p.wts[d0:d1].double() if p.wts is not None else 1.0
        Wpx = W * p.det_w[d0:d1, None] * px
        return [Wpx * sw[d0:d1, k : k + 1] for k in range(S)]

    acc, mag = _scatter(p, pix, S, terms)
    _exact(mag, 9)
    return acc


def test_case_e_normal_operator_nearest(gpu_ctx, case_b):
    """E: mrx_map_normal_apply (16-byte entries, normal_accumulate_kernel) with sample and detector weights, three Stokes
    planes and two channels: routed with the full buffer and with three chunks, the atomic form (d_work = NULL) and the
    reference, bit for bit."""
    import torch

    p = case_b
    pix = _pixels(gpu_ctx, p)
    x = p.dyadic_map(p.S)
    ref = _ref_normal(p, pix, x)
    _equal(_normal(gpu_ctx, p, x, None), ref, "atomic")
    geo = p.geometry(16)
    for wb in (geo.full_bytes, three_chunk_bytes(geo)):
        g = p.geometry(16, wb)
        _report(f"E nearest ({len(g.chunks)} chunks)", g, _max_segments(p, pix, g))
        _equal(_normal(gpu_ctx, p, x, _work(wb)), ref, f"routed, {len(g.chunks)} chunks")
    torch.cuda.synchronize()


def test_case_e_normal_operator_bilinear(gpu_ctx):
    """E: the bilinear normal operator at case C's geometry, three Stokes planes: routed (full buffer, three chunks)
    against the atomic form to float64 rounding, and <x, P^T W P x> = sum W (P x)^2 with P x from mrx_map_project."""
    import torch

    from maria_amd._lib import ptr

    p = Problem("C", seed=5, weights=True, fov_deg=0.4, S=3, tod=False)
    x = p.dyadic_map(3)
    atomic = _normal(gpu_ctx, p, x, None)
    geo = p.geometry(16)
    for wb in (geo.full_bytes, three_chunk_bytes(geo)):
        _check_bilinear([atomic], [_normal(gpu_ctx, p, x, _work(wb))], wb)
    px = torch.empty((p.D, p.T), dtype=torch.float32, device=DEV)
    gpu_ctx.call("mrx_map_project", C.byref(p.sky()), ptr(x), *p.point(), 1.0, 0.0, ptr(px), px.stride(0))
    quad = float((p.wts.double() * p.det_w[:, None] * px.double() ** 2).sum())
    got = float((x * atomic).sum())
    assert quad > 0 and abs(got - quad) <= 1e-6 * quad, (got, quad)


@pytest.mark.parametrize("L", [50, 1500])
def test_case_f_baselines(gpu_ctx, case_b, L):
    """F: the destriper's P^T W F a (mrx_bin_map_baselines, baseline_bucket_kernel): baselines of 50 and 1500 samples --
    across tile edges, T % L != 0 -- routed (full buffer, three chunks) against the atomic form and the reference."""
    import torch

    from maria_amd._lib import ptr

    p = case_b
    assert p.T % L
    nb = -(-p.T // L)
    amp = torch.empty((p.D, nb), dtype=torch.float64, device=DEV).random_(-64, 65, generator=p.gen).div_(16)
    pix = _pixels(gpu_ctx, p)
    base = torch.arange(p.T, device=DEV) // L

    def terms(d0, d1, idx):
        v = p.wts[d0:d1].double() * p.det_w[d0:d1, None] * amp[d0:d1][:, base]
        return [v * p.sw[d0:d1, k : k + 1] for k in range(p.S)]

    ref, mag = _scatter(p, pix, p.S, terms)
    _exact(mag, 8)
    del pix

    def run(work):
        y = torch.zeros_like(ref)
        gpu_ctx.call("mrx_bin_map_baselines", C.byref(p.sky()), ptr(amp), L, *p.weight_args(), ptr(p.det_w), *p.point(), ptr(y),
                     ptr(work), 0 if work is None else work.numel())
        return y

    _equal(run(None), ref, "atomic")
    geo = p.geometry(16)
    for wb in (geo.full_bytes, three_chunk_bytes(geo)):
        _equal(run(_work(wb)), ref, f"routed, {len(p.geometry(16, wb).chunks)} chunks")


def test_case_g_blocks(gpu_ctx, case_b):
    """G: the blocks of P^T W P (mrx_bin_map_blocks, atomic only) at case B's geometry, bit for bit."""
    import torch

    from maria_amd._lib import ptr

    p = case_b
    pairs = [(k, l) for k in range(p.S) for l in range(k, p.S)]
    pix = _pixels(gpu_ctx, p)

    def terms(d0, d1, idx):
        Wd = p.wts[d0:d1].double() * p.det_w[d0:d1, None]
        return [Wd * (p.sw[d0:d1, k] * p.sw[d0:d1, l])[:, None] for k, l in pairs]

    ref, mag = _scatter(p, pix, len(pairs), terms)
    _exact(mag, 5)
    H = torch.zeros_like(ref)
    gpu_ctx.call("mrx_bin_map_blocks", C.byref(p.sky()), *p.weight_args(), ptr(p.det_w), *p.point(), ptr(H))
    _equal(H, ref, "blocks")


def test_case_j_benchmark_geometry(gpu_ctx):
    """J: scripts/mlmap_bench.py's shape -- 10 000 detectors x 240 000 samples of a daisy at 400 Hz onto 1024^2, R = 512,
    pass-B ranges of 1148 tiles (five batches) -- at the buffer the mappers pick: the binning without weights in one
    chunk and the nearest normal operator with three Stokes planes in two, against a float64 reference, bit for bit."""
    import torch

    from maria_amd import mappers

    need = 60 << 30
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < need:
        pytest.skip(f"needs {need >> 30} GiB of free device memory, {free >> 30} GiB free")
    n = 1024
    p = Problem("J", seed=7, weights=False, fov_deg=1.0)
    step = 0.05 / n  # mlmap_bench's grid
    p.eta0, p.deta, p.xi0, p.dxi = 0.025, -step, -0.025, step
    p.centre = (float(np.mean(p.az.cpu().numpy())), float(np.mean(p.el.cpu().numpy())))
    pix = _pixels(gpu_ctx, p)
    ref_sum, ref_wgt = _ref_binning(p, pix)
    lo, full = C.c_size_t(), C.c_size_t()
    assert gpu_ctx.lib.mrx_bin_map_work_bytes(C.byref(p.sky()), p.D, p.T, C.byref(lo), C.byref(full)) == 0
    wb = mappers._work_bytes(lo.value, full.value, torch.device(DEV))
    geo = p.geometry(8, wb)
    _report("J binning", geo, _max_segments(p, pix, geo))
    assert geo.R == 512 and len(geo.chunks) == 1 and geo.chunks[0].per > 1000 and geo.chunks[0].batches == 5
    work = _work(wb)
    got = _bin(gpu_ctx, p, routed=True, work=work)
    del work
    _equal(got[0], ref_sum, "routed sum")
    _equal(got[1], ref_wgt, "routed weight")
    del got, ref_sum, ref_wgt
    p.tod = None
    torch.cuda.empty_cache()
    sw3 = _pick(SW_VALUES, (p.D, 3), p.gen, torch.float64)
    x = p.dyadic_map(3)
    ref = _ref_normal(p, pix, x, sw=sw3)
    assert gpu_ctx.lib.mrx_map_normal_work_bytes(C.byref(p.sky(S=3)), p.D, p.T, C.byref(lo), C.byref(full)) == 0
    wb = mappers._work_bytes(lo.value, full.value, torch.device(DEV))
    geo = p.geometry(16, wb)
    _report("J normal operator", geo, _max_segments(p, pix, geo))
    assert len(geo.chunks) == 2 and all(ch.per > 256 for ch in geo.chunks)
    del pix
    torch.cuda.empty_cache()
    work = _work(wb)
    y = _normal(gpu_ctx, p, x, work, sw=sw3, S=3)
    del work
    _equal(y, ref, "routed normal operator")
    del y, ref
    torch.cuda.empty_cache()


def test_case_k_mapper_level(gpu_ctx, monkeypatch):
    """K: BinMapper on a dyadic TOD (polarisation angles 0: the Mueller rows 1/2, 1/2, 0 are exact) -- the full buffer,
    a BIN_WORK_LIMIT_BYTES that makes the call walk the time axis in chunks, and the atomic form -- the same map, bit
    for bit."""
    import functools

    import torch

    from maria_amd import mappers, synthetic
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    D, T = 600, 60_000
    t = 1.7e9 + np.arange(T) / 400.0
    az, el = synthetic.daisy_scan(t)
    off = synthetic.hex_pack(D, np.radians(0.4))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    tod = torch.empty((D, T), dtype=torch.float32, device=DEV).random_(-1024, 1025, generator=gen).mul_(0.125)
    dets = Detectors(off, [Band(center=150e9, width=30e9, name="f150")], gamma=np.zeros(D))
    data = TOD({"map": tod}, dets, Coordinates(t, az, el, offsets=off), units="K_RJ")
    kw = dict(center=(45.0, 60.0), width=1.6, resolution=1.6 / 300, frame="az/el", stokes="IQU", units="K_RJ")

    def run():
        m = mappers.BinMapper([data], **kw)
        m.run()
        return m

    m = run()
    full = m.products
    # a buffer of three columns of 16-byte entries: chunks of five columns of 8-byte ones
    shape = (len(m.nu), m.n_eta, m.n_xi, D, T, False, 8)
    geo = routed_geometry(*shape, 3 * routed_geometry(*shape).min_bytes)
    print(f"\nK: {m.n_eta} x {m.n_xi}, R {geo.R}, {len(geo.chunks)} chunks of {[ch.nc for ch in geo.chunks]} columns")
    assert len(geo.chunks) > 3 and geo.chunks[-1].nc < geo.chunks[0].nc
    monkeypatch.setattr(mappers, "BIN_WORK_LIMIT_BYTES", 3 * geo.min_bytes)
    chunked = run().products
    monkeypatch.setattr(mappers, "bin_map", functools.partial(mappers.bin_map, bucketed=False))
    atomic = run().products
    assert full["weight"].shape == (3, 1, m.n_eta, m.n_xi) and full["weight"][0].sum() > 0 and np.abs(full["sum"]).max() > 0
    assert 128 * np.abs(full["weight"]).max() < 2.0 ** (53 - 4)  # sum |W d sw| <= max |d| sum W |sw|: exact (q = 3 + 1)
    for key in ("sum", "weight"):
        np.testing.assert_array_equal(chunked[key], full[key])
        np.testing.assert_array_equal(atomic[key], full[key])
