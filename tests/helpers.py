"""Shared builders for the tests: problems with numpy screens attached."""

from __future__ import annotations

import numpy as np

from maria_amd import synthetic
from oracle import hotpath, screens


def attach_numpy_screens(problem, seed=0, smooth=True):
    rng = np.random.default_rng(seed)
    for layer in problem["layers"]:
        ne, nc = len(layer["extrusion"]), len(layer["cross_section"])
        de = layer["extrusion"][1] - layer["extrusion"][0]
        dc = layer["cross_section"][1] - layer["cross_section"][0]
        v = screens.numpy_screen(ne, nc, de, dc, layer["r0"], layer["nu"], rng)
        if smooth:
            v = hotpath.smooth_screen(v, layer["beam_sigma"] / de, layer["beam_sigma"] / dc)
        layer["values"] = np.asarray(v, np.float32)
    return problem


def small_problem(**kw):
    args = dict(n_det=67, n_bands=2, fov_deg=0.5, fs=50.0, duration=20.0, n_layers=3, side=128, t0=1.7e9)
    args.update(kw)
    return attach_numpy_screens(synthetic.make_problem(**args))


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


# ---- the routed map operators' launch geometry (tests/test_gpu_map_routed.py, tests/test_host_map_routed.py) ----
# A mirror of bin_regions, bin_geometry, mrx_bin_map_work_bytes and routed_bin in maria_amd/csrc/mrx_map.hip: what pass A
# and pass B are launched over for a map, a TOD shape, an entry size (8: nearest pixel without weights, 12: with weights,
# 16: bilinear, and every form of the normal operator and the baselines) and a work buffer.
BIN_REGION = (32, 64)   # pixels of a map region: eta x xi
BIN_MAX_REGIONS = 2048
BIN_BATCH = 256         # tiles pass B lists per batch (kBlock)


def _ceil(a, b):
    return -(-a // b)


def routed_geometry(C, n_eta, n_xi, D, T, bilinear, entry_bytes, work_bytes=None):
    """The chunks, splits and batches of one routed call; work_bytes None: mrx_bin_map_work_bytes' full size."""
    from types import SimpleNamespace

    nby, nbx = _ceil(n_eta, BIN_REGION[0]), _ceil(n_xi, BIN_REGION[1])
    R = C * nby * nbx
    assert R <= BIN_MAX_REGIONS, "the routed form takes at most 2048 regions"
    tile_det, tile_samples = (8, 256) if bilinear else (16, 1024)
    tile_entries = tile_det * tile_samples * (4 if bilinear else 1)
    tiles_y = _ceil(D, tile_det)
    min_bytes = tiles_y * (tile_entries * 16 + R * 4)  # the sizing functions' column: 16-byte entries
    cols_total = _ceil(T, tile_samples)
    full_bytes = min_bytes * cols_total
    col = tiles_y * (tile_entries * entry_bytes + R * 4)
    wb = full_bytes if work_bytes is None else work_bytes
    assert wb >= col, "below one column of tiles"
    cols = min(wb // col, cols_total)
    halved = 0
    while cols * tiles_y * tile_entries > (1 << 32) - 1:  # pass B indexes a chunk's entries with 32 bits
        cols, halved = (cols + 1) // 2, halved + 1
    splits = max(1, 65536 // R)
    chunks = []
    for c0 in range(0, cols_total, cols):
        nc = min(cols, cols_total - c0)
        n_tiles = nc * tiles_y
        sp = min(splits, n_tiles)
        per = _ceil(n_tiles, sp)
        chunks.append(SimpleNamespace(c0=c0, nc=nc, s0=c0 * tile_samples, s1=min((c0 + nc) * tile_samples, T), n_tiles=n_tiles,
                                      sp=sp, per=per, batches=_ceil(per, BIN_BATCH), entries=n_tiles * tile_entries))
    return SimpleNamespace(R=R, nby=nby, nbx=nbx, tile_det=tile_det, tile_samples=tile_samples, tile_entries=tile_entries,
                           tiles_y=tiles_y, col=col, min_bytes=min_bytes, full_bytes=full_bytes, cols_total=cols_total, cols=cols,
                           halved=halved, splits=splits, chunks=chunks, regions_per_thread=_ceil(R, BIN_BATCH))


def three_chunk_bytes(q):
    """A work buffer of two fifths of the time axis' columns (of the call's own entry size): three chunks, the last ragged."""
    return (2 * q.cols_total // 5) * q.col


# The cases of tests/test_gpu_map_routed.py: map (channels, Stokes planes, n_eta x n_xi), TOD (D x T), pointing, entry size.
ROUTED_CASES = {
    # nearest pixel without weights (BinMapper's default): R = 288 > 256 regions, two per thread in pass A's scan
    "A": dict(C=1, S=1, n_eta=512, n_xi=1100, D=2000, T=100_000, bilinear=False, entry_bytes=8),
    # nearest with weights: R = 2048 with partial regions on both far edges, per = 290 (two batches), last tile row of 8
    "B": dict(C=2, S=3, n_eta=1000, n_xi=2040, D=1000, T=150_001, bilinear=False, entry_bytes=12),
    # bilinear: R = 1081, odd and > 1024, per = 493
    "C": dict(C=1, S=2, n_eta=1500, n_xi=1470, D=500, T=120_000, bilinear=True, entry_bytes=16),
    # one-column chunks (the sizing functions' minimum buffer) on a small shape
    "D1": dict(C=2, S=2, n_eta=200, n_xi=300, D=200, T=20_000, bilinear=False, entry_bytes=12),
    # scripts/mlmap_bench.py's geometry: 10 000 x 240 000 onto 1024^2
    "J": dict(C=1, S=1, n_eta=1024, n_xi=1024, D=10_000, T=240_000, bilinear=False, entry_bytes=8),
}
