"""The Gaussian stencil's launch routes restated, and the cases that reach each of them.

`plan` repeats in Python what the host code of maria_amd/csrc/mrx_gauss.hip decides for one call of
mrx_gauss_smooth2d: the radius per axis, the route of the y pass (skipped, direct, through the transposed plane), the
kernel instance and tile of every pass, which tiles are staged without the reflect fold ("interior"), and refusal.
`CASES` is the table tests/test_gpu_gauss_edges.py runs; every case names the branches it is there for (`reaches`), and
tests/test_host_gauss_cases.py checks those claims against `plan` without a GPU.  numpy and scipy only.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import scipy.ndimage

# ---- the constants of mrx_gauss.hip ----
K_BLOCK = 256
X_PER_THREAD = 4
X_COLS = K_BLOCK * X_PER_THREAD  # outputs of a row per workgroup of the x pass
X_ROWS = 4                       # rows per workgroup of the x pass
Y_COLS = 64
ACC_BLOCK = 16
MAX_LDS = 128 * 1024
TRANSPOSE_RADIUS = 64
TAP_SLOTS = 32                   # mrx_ctx::kTapSlots

# the bounds the project promises, max|got - ref| / max(1, max|ref|), per MRX_OPT_GAUSS_ACCUM
BOUND = {1: 2.5e-7, 2: 1.0e-6, 0: 1.0e-6}


def radius_of(sigma, truncate=4.0):
    return int(truncate * sigma + 0.5)


def x_lds_bytes(radius):
    return X_ROWS * ((X_COLS + 2 * radius + 4 + ACC_BLOCK + 3) & ~3) * 4


def y_tile(radius):
    """(tile_rows, outputs per thread, LDS bytes) of the direct y pass (smooth_axis0)."""
    def image(rows, per_thread):
        return (rows + 2 * radius + ACC_BLOCK + per_thread) * Y_COLS * 4

    tile_rows = 64
    while tile_rows > 32 and image(tile_rows, 8) > 40 * 1024:
        tile_rows //= 2
    if image(tile_rows, 8) > MAX_LDS:
        tile_rows = 16
    per_thread = 8 if tile_rows >= 32 else 4
    return tile_rows, per_thread, image(tile_rows, per_thread)


def _largest(accepts):
    r = 0
    while accepts(r + 1):
        r += 1
    return r


MAX_X_RADIUS = _largest(lambda r: x_lds_bytes(r) <= MAX_LDS)
MAX_Y_RADIUS = _largest(lambda r: y_tile(r)[2] <= MAX_LDS)
MIN_Y_ROWS4_RADIUS = next(r for r in range(MAX_Y_RADIUS + 1) if y_tile(r)[1] == 4)


def tiles(n, radius, tile):
    """Per tile along an axis of n pixels: staged without the reflect fold?"""
    return [t0 - radius >= 0 and t0 + tile + radius <= n for t0 in range(0, n, tile)]


def blocked(mode, radius):
    return mode == 2 or (mode == 0 and radius >= 16)


def _x_pass(axis, n_along, radius, mode, transposed=False):
    refused = x_lds_bytes(radius) > MAX_LDS
    b = blocked(mode, radius)
    return SimpleNamespace(axis=axis, transposed=transposed, radius=radius, blocked=b, kernel=f"gauss_x_kernel<{str(b).lower()}>",
                           tile=X_COLS, tile_rows=None, tiles=tiles(n_along, radius, X_COLS), refused=refused)


def plan(ny, nx, sigma_y, sigma_x, truncate=4.0, mode=0):
    """What mrx_gauss_smooth2d launches: .ry, .rx, .route_y ("skip" | "direct" | "transposed"), .do_x, .passes (in launch
    order, up to and including a refused one) and .refused (None, or the axis named by the error message)."""
    do_y, do_x = sigma_y > 1e-15, sigma_x > 1e-15
    ry = radius_of(sigma_y, truncate) if do_y else None
    rx = radius_of(sigma_x, truncate) if do_x else None
    passes = []
    route_y = "skip"
    if do_y:
        if ry >= TRANSPOSE_RADIUS and ny <= 65535 * 64 and nx <= 65535 * X_ROWS:
            route_y = "transposed"
            passes.append(_x_pass("y", ny, ry, mode, transposed=True))
        else:
            route_y = "direct"
            tile_rows, per_thread, lds = y_tile(ry)
            b = blocked(mode, ry)
            passes.append(SimpleNamespace(axis="y", transposed=False, radius=ry, blocked=b,
                                          kernel=f"gauss_y_kernel<{str(b).lower()}, {per_thread}>", tile=tile_rows,
                                          tile_rows=tile_rows, tiles=tiles(ny, ry, tile_rows), refused=lds > MAX_LDS))
    if do_x and not (passes and passes[-1].refused):
        passes.append(_x_pass("x", nx, rx, mode))
    refused = None
    if passes and passes[-1].refused:
        # (a y radius refused on the transposed route is refused by the x pass, and the message names x)
        refused = "x" if passes[-1].kernel.startswith("gauss_x") else "y"
    return SimpleNamespace(ry=ry, rx=rx, route_y=route_y, do_x=do_x, passes=passes, refused=refused)


def reference(a, sigma_y, sigma_x, truncate=4.0):
    return scipy.ndimage.gaussian_filter(np.asarray(a, np.float32), sigma=(sigma_y, sigma_x), truncate=truncate)


# ---- the branches of the dispatch, by name: a predicate on (case, plan) ----
def _pass(p, axis):
    return next((q for q in p.passes if q.axis == axis), None)


def _has(p, axis, **want):
    q = _pass(p, axis)
    return q is not None and all(getattr(q, k) == v for k, v in want.items())


BRANCHES = {
    "x_interior": lambda c, p: _has(p, "x") and any(_pass(p, "x").tiles) and p.refused is None,
    "x_interior_exact": lambda c, p: _has(p, "x", blocked=False) and any(_pass(p, "x").tiles),
    "x_interior_blocked": lambda c, p: _has(p, "x", blocked=True) and any(_pass(p, "x").tiles),
    # (3100 columns are four tiles: the rim, two interior ones, and a ragged rim of 28 columns)
    "x_rim_interior_ragged_rim": lambda c, p: _has(p, "x") and _pass(p, "x").tiles == [False, True, True, False] and c["shape"][1] % X_COLS != 0,
    "transposed_interior": lambda c, p: p.route_y == "transposed" and any(_pass(p, "y").tiles),
    "y_rows4": lambda c, p: p.route_y == "direct" and _pass(p, "y").kernel.endswith(", 4>") and p.refused is None,
    "refuse_x": lambda c, p: p.refused == "x" and _pass(p, "x").radius == MAX_X_RADIUS + 1,
    "refuse_y": lambda c, p: p.refused == "y" and p.ry == MAX_Y_RADIUS + 1,
    "max_radius_x": lambda c, p: p.refused is None and p.rx == MAX_X_RADIUS,
    "max_radius_y": lambda c, p: p.refused is None and p.route_y == "direct" and p.ry == MAX_Y_RADIUS,
    "truncate_not_4": lambda c, p: c["truncate"] != 4.0,
    "radius_0": lambda c, p: 0 in (p.ry, p.rx),
    "radius_1_from_sigma_0.125": lambda c, p: 0.125 in (c["sy"], c["sx"]) and 1 in (p.ry, p.rx),
    "switch_direct_63": lambda c, p: p.route_y == "direct" and p.ry == 63 and _pass(p, "y").tile_rows == 32,
    "switch_transposed_64": lambda c, p: p.route_y == "transposed" and p.ry == 64,
    "tap_cache_wrap_evict_key": lambda c, p: c["kind"] == "tapcache",
    "nonfinite": lambda c, p: c["kind"] == "nonfinite",
}

ALL_MODES = (1, 2, 0)


def _case(name, kind, shape, sy, sx, reaches, truncate=4.0, modes=ALL_MODES, inplace=True, twin=None, **extra):
    return dict(name=name, kind=kind, shape=shape, sy=sy, sx=sx, truncate=truncate, modes=modes, inplace=inplace,
                reaches=tuple(reaches), twin=twin, **extra)


def _px(y, x, *touches):
    return dict(y=y, x=x, touches=frozenset(touches))


_X_PIXELS = [_px(45, 3, "left"), _px(45, 1021), _px(45, 1022), _px(45, 1023), _px(45, 1024)]
_Y_PIXELS = [_px(3, 550, "top"), _px(45, 1023), _px(50, 1024)]

CASES = [
    # x interior tiles: the smallest width with one, and the twin one column narrower with none
    _case("x_int_r8", "finite", (6, 2048 + 8), 0.0, 2.0, ["x_interior", "x_interior_exact"], twin="x_rim_r8"),
    _case("x_rim_r8", "finite", (6, 2047 + 8), 0.0, 2.0, []),
    _case("x_int_r20", "finite", (6, 2048 + 20), 0.0, 5.0, ["x_interior", "x_interior_blocked"], twin="x_rim_r20"),
    _case("x_rim_r20", "finite", (6, 2047 + 20), 0.0, 5.0, []),
    _case("x_four_tiles_s2", "finite", (5, 3100), 2.0, 2.0, ["x_interior", "x_rim_interior_ragged_rim"], twin="x_rim_r8"),
    _case("x_four_tiles_s5", "finite", (5, 3100), 5.0, 5.0, ["x_interior", "x_rim_interior_ragged_rim"], twin="x_rim_r20"),
    # the transposed route with an interior tile (of the transposed plane's rows), and its twin
    _case("t_int_sx0", "finite", (2200, 7), 16.0, 0.0, ["transposed_interior"], twin="t_rim"),
    _case("t_int_sx1", "finite", (2200, 7), 16.0, 1.0, ["transposed_interior"], twin="t_rim"),
    _case("t_rim", "finite", (2111, 70), 16.0, 0.0, []),
    # the switch between the direct and the transposed y pass on one plane
    _case("switch_r63", "finite", (130, 70), 15.75, 0.0, ["switch_direct_63"]),
    _case("switch_r64", "finite", (130, 70), 16.0, 0.0, ["switch_transposed_64"]),
    # gauss_y_kernel<*, 4>: only where the transposed route is refused (nx > 65535 * 4)
    _case("y_rows4_r232", "finite", (24, 262141), 58.0, 0.0, ["y_rows4"], modes=(1, 2), inplace=False),
    # the largest radii and one more
    _case("max_rx", "finite", (3, 40), 0.0, MAX_X_RADIUS / 4.0, ["max_radius_x"]),
    _case("max_ry", "finite", (24, 262141), MAX_Y_RADIUS / 4.0, 0.0, ["max_radius_y", "y_rows4"], modes=(1, 2), inplace=False),
    _case("over_rx", "refuse", (3, 40), 0.0, (MAX_X_RADIUS + 1) / 4.0, ["refuse_x"]),
    _case("over_ry", "refuse", (24, 262141), (MAX_Y_RADIUS + 1) / 4.0, 0.0, ["refuse_y"]),
    # radius 0 (one tap: the input's bits), the first sigma with radius 1, and truncate != 4
    _case("r0_x_0.1", "bits", (37, 70), 0.0, 0.1, ["radius_0"]),
    _case("r0_y_0.1", "bits", (37, 70), 0.1, 0.0, ["radius_0"]),
    _case("r0_x_0.124", "bits", (37, 70), 0.0, 0.124, ["radius_0"]),
    _case("r0_y_0.124", "bits", (37, 70), 0.124, 0.0, ["radius_0"]),
    _case("r0_both", "bits", (37, 70), 0.124, 0.1, ["radius_0"]),
    _case("r1_0.125", "finite", (37, 70), 0.125, 0.125, ["radius_1_from_sigma_0.125"]),
    _case("trunc_2.0", "finite", (37, 70), 2.0, 2.0, ["truncate_not_4"], truncate=2.0),
    _case("trunc_3.3", "finite", (37, 70), 2.0, 2.0, ["truncate_not_4"], truncate=3.3),
    _case("trunc_6.0", "finite", (37, 70), 2.0, 2.0, ["truncate_not_4"], truncate=6.0),
    # the tap cache: 40 keys through 32 slots, the first again (evicted), one sigma under truncate 3, 4, 3
    _case("tap_cache", "tapcache", (33, 70), 0.0, 0.0, ["tap_cache_wrap_evict_key"],
          calls=tuple((0.5 + 0.11 * i, 4.0) for i in range(40)) + ((0.5, 4.0), (2.25, 3.0), (2.25, 4.0), (2.25, 3.0))),
    # one non-finite pixel: along x (exact and blocked radii; the reflecting edge, both sides of the tile boundary at
    # column 1024, every residue of the column mod 4), along y directly (rows of two residues mod 8, across the y tiles'
    # boundary at row 64), both, and along y through the transposed plane (the row is its column there)
    _case("nf_x_r12", "nonfinite", (100, 1100), 0.0, 3.0, ["nonfinite"], pixels=_X_PIXELS),
    _case("nf_x_r20", "nonfinite", (100, 1100), 0.0, 5.0, ["nonfinite"], pixels=_X_PIXELS),
    _case("nf_y_r12", "nonfinite", (100, 1100), 3.0, 0.0, ["nonfinite"], pixels=_Y_PIXELS),
    _case("nf_y_r20", "nonfinite", (100, 1100), 5.0, 0.0, ["nonfinite"], pixels=_Y_PIXELS),
    _case("nf_yx", "nonfinite", (100, 1100), 3.0, 5.0, ["nonfinite"], pixels=[_px(3, 3, "top", "left"), _px(45, 1023), _px(50, 1022)]),
    _case("nf_t_r64", "nonfinite", (200, 80), 16.0, 0.0, ["nonfinite"],
          pixels=[_px(5, 40, "top"), _px(100, 40), _px(101, 40), _px(102, 40), _px(103, 40)]),
    _case("nf_t_r64_x", "nonfinite", (200, 80), 16.0, 3.0, ["nonfinite"], pixels=[_px(100, 40), _px(103, 41)]),
]
BY_NAME = {c["name"]: c for c in CASES}
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)
NONFINITE_MARGIN = 24  # finite pixels between scipy's non-finite set and every edge the pixel does not touch on purpose


def cases(kind):
    return [c for c in CASES if c["kind"] == kind]


def case_plan(c, mode=0):
    ny, nx = c["shape"]
    return plan(ny, nx, c["sy"], c["sx"], c["truncate"], mode)


def reaches(c, branch):
    """Does the case reach the branch in at least one of the modes it runs?"""
    return any(BRANCHES[branch](c, case_plan(c, m)) for m in c["modes"])


_inputs = {}


def case_input(shape, seed=11):
    """White noise of a shape, made once and shared (read-only) by the cases on that plane."""
    key = (tuple(shape), seed)
    if key not in _inputs:
        a = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def nonfinite_input(c, pixel, value):
    a = case_input(c["shape"]).copy()
    a[pixel["y"], pixel["x"]] = value
    return a


_refs = {}


def case_reference(c):
    """scipy's result of a finite case on case_input(shape): computed once, read-only."""
    key = (c["shape"], c["sy"], c["sx"], c["truncate"])
    if key not in _refs:
        r = reference(case_input(c["shape"]), c["sy"], c["sx"], c["truncate"])
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]
