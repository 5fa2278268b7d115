"""CPU tier: the launch arithmetic that tests/test_gpu_map_routed.py mirrors (helpers.routed_geometry) against the library's
own sizing functions, and the geometry each of its cases claims -- so that no case can quietly shrink into one where every
pass-B workgroup reads one segment of one tile."""

import ctypes as C

import pytest

from helpers import ROUTED_CASES, routed_geometry, three_chunk_bytes
from maria_amd import _lib


def _sky(c, bilinear=None):
    bil = c["bilinear"] if bilinear is None else bilinear
    return _lib.MrxSkyMap(None, c["C"], c["S"], c["n_eta"], c["n_xi"], 1.0, -1e-4, -1.0, 1e-4, 0.8, 1.0, int(bil), 0)


@pytest.mark.parametrize("name", sorted(ROUTED_CASES))
@pytest.mark.parametrize("bilinear", [False, True])
def test_sizes_match_the_library(name, bilinear):
    """The helper's column (one column of tiles of 16-byte entries) and full size are mrx_bin_map_work_bytes' and
    mrx_map_normal_work_bytes' own, for both tile shapes (16 x 1024 nearest, 8 x 256 bilinear)."""
    lib = _lib.load()
    c = ROUTED_CASES[name]
    q = routed_geometry(c["C"], c["n_eta"], c["n_xi"], c["D"], c["T"], bilinear, 16)
    for fn in (lib.mrx_bin_map_work_bytes, lib.mrx_map_normal_work_bytes):
        lo, full = C.c_size_t(), C.c_size_t()
        assert fn(C.byref(_sky(c, bilinear)), c["D"], c["T"], C.byref(lo), C.byref(full)) == 0
        assert (lo.value, full.value) == (q.min_bytes, q.full_bytes), (name, fn.__name__)
    # an odd shape of every kind: ragged detector rows, ragged tile columns, partial regions
    for D, T in [(1, 1), (17, 1025), (9, 257), (1001, 3 * 1024 + 1)]:
        q = routed_geometry(2, 33, 65, D, T, bilinear, 16)
        lo, full = C.c_size_t(), C.c_size_t()
        sky = _lib.MrxSkyMap(None, 2, 1, 33, 65, 1.0, -1e-4, -1.0, 1e-4, 0.8, 1.0, int(bilinear), 0)
        assert lib.mrx_bin_map_work_bytes(C.byref(sky), D, T, C.byref(lo), C.byref(full)) == 0
        assert (lo.value, full.value) == (q.min_bytes, q.full_bytes) and q.R == 2 * 2 * 2


def test_case_geometry_claims():
    """What each GPU case exists for, from the launcher's arithmetic alone."""
    g = lambda c, **kw: routed_geometry(c["C"], c["n_eta"], c["n_xi"], c["D"], c["T"], c["bilinear"], c["entry_bytes"], **kw)  # noqa: E731
    A, B, Cb, D1, J = (ROUTED_CASES[k] for k in ("A", "B", "C", "D1", "J"))
    a = g(A)
    assert a.R == 288 and a.regions_per_thread == 2 and len(a.chunks) == 1 and a.chunks[0].per > 1
    b = g(B)
    assert b.R == 2048 and B["D"] % 16 == 8 and B["n_eta"] % 32 and B["n_xi"] % 64  # partial regions on both far edges
    assert len(b.chunks) == 1 and b.chunks[0].per == 290 and b.chunks[0].batches == 2
    c = g(Cb)
    assert c.R == 1081 and c.R % 2 == 1 and c.R > 1024 and c.chunks[0].per > 256 and c.chunks[0].batches == 2
    # two fifths of the columns a chunk: three chunks, the last one ragged
    for case, q in ((A, a), (B, b), (Cb, c)):
        three = g(case, work_bytes=three_chunk_bytes(q))
        n = three.chunks[0].nc
        assert [ch.nc for ch in three.chunks] == [n, n, q.cols_total - 2 * n] and 0 < q.cols_total - 2 * n < n
        assert three.chunks[-1].s1 == case["T"] and all(x.s1 == y.s0 for x, y in zip(three.chunks, three.chunks[1:]))
    # the sizing functions' minimum: one column a chunk
    d1 = g(D1, work_bytes=g(D1).min_bytes)
    assert d1.cols == 1 and len(d1.chunks) == d1.cols_total == 20
    # the benchmark's geometry at the mappers' 24 GiB cap: R = 512, per = 1148 (five batches); 16-byte entries in two chunks
    j8 = g(J, work_bytes=24 << 30)
    assert j8.R == 512 and j8.splits == 128 and len(j8.chunks) == 1 and j8.chunks[0].per == 1148 and j8.chunks[0].batches == 5
    j16 = routed_geometry(1, 1024, 1024, 10_000, 240_000, False, 16, 24 << 30)
    assert len(j16.chunks) == 2 and min(ch.per for ch in j16.chunks) > 256
    # bilinear binning at that size within the cap: about seven chunks
    jb = routed_geometry(1, 1024, 1024, 10_000, 240_000, True, 16, 24 << 30)
    assert len(jb.chunks) == 7


def test_chunks_halve_below_2_to_the_32_entries():
    """routed_bin halves the columns of a chunk until pass B's 32-bit entry index holds (nearest, 8-byte entries: a buffer
    of 34 GB and more)."""
    D, T = 20_000, 300 * 1024
    q = routed_geometry(1, 1024, 1024, D, T, False, 8, 64 << 30)
    assert q.cols_total == 300 and q.halved == 1 and q.cols == 150 and len(q.chunks) == 2
    assert all(ch.entries <= (1 << 32) - 1 for ch in q.chunks)
    # just below the cap: no halving
    q = routed_geometry(1, 1024, 1024, 16 * 1024, 255 * 1024, False, 8, 64 << 30)
    assert q.halved == 0 and q.chunks[0].entries == 1024 * 255 * 16384 < 1 << 32
