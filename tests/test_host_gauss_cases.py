"""The Gaussian stencil's case table (tests/gauss_cases.py) against its restatement of the dispatch: every branch the
table is there for is reached by a case that names it, every interior-tile case has a twin just too narrow for one, and
the non-finite cases leave room to see a kernel that spreads further than scipy.  Runs without a GPU."""

import numpy as np
import pytest

import gauss_cases as gc


def test_limits_follow_from_the_lds_budget():
    """The largest radii from kMaxLds and the kernels' LDS images; the y pass changes instance on the way."""
    assert gc.x_lds_bytes(gc.MAX_X_RADIUS) <= gc.MAX_LDS < gc.x_lds_bytes(gc.MAX_X_RADIUS + 1)
    assert gc.y_tile(gc.MAX_Y_RADIUS)[2] <= gc.MAX_LDS < gc.y_tile(gc.MAX_Y_RADIUS + 1)[2]
    assert (gc.MAX_X_RADIUS, gc.MAX_Y_RADIUS, gc.MIN_Y_ROWS4_RADIUS) == (3574, 238, 229)
    assert [gc.y_tile(r)[:2] for r in (0, 36, 37, 228, 229, 238)] == [(64, 8), (64, 8), (32, 8), (32, 8), (16, 4), (16, 4)]


@pytest.mark.parametrize("branch", sorted(gc.BRANCHES))
def test_every_branch_is_reached_by_a_case_that_names_it(branch):
    named = [c for c in gc.CASES if branch in c["reaches"]]
    assert named, f"no case of the table names {branch}"
    for c in named:
        assert gc.reaches(c, branch), (c["name"], branch)


def test_every_named_branch_exists():
    for c in gc.CASES:
        assert set(c["reaches"]) <= set(gc.BRANCHES), c["name"]
        assert c["kind"] in ("finite", "bits", "refuse", "tapcache", "nonfinite") and set(c["modes"]) <= {0, 1, 2}


def test_removing_a_case_is_noticed():
    """The check above is by name: without its only case a branch is unreached."""
    for branch in ("y_rows4", "refuse_y", "switch_direct_63", "tap_cache_wrap_evict_key"):
        only = [c for c in gc.CASES if branch in c["reaches"]]
        rest = [c for c in gc.CASES if c not in only]
        assert only and not any(branch in c["reaches"] for c in rest)


def _interior_pass(p):
    return next(q for q in p.passes if any(q.tiles))


@pytest.mark.parametrize("case", [c for c in gc.CASES if any(b in c["reaches"] for b in ("x_interior", "transposed_interior"))],
                         ids=lambda c: c["name"])
def test_interior_cases_have_a_twin_without(case):
    for mode in case["modes"]:
        q = _interior_pass(gc.case_plan(case, mode))
        n = case["shape"][0] if q.transposed else case["shape"][1]
        smallest = 2 * gc.X_COLS + q.radius  # the second tile is the first that can lie inside: x0 = 1024 >= r, x0 + 1024 + r <= n
        assert n >= smallest and not any(gc.tiles(smallest - 1, q.radius, gc.X_COLS)) and any(gc.tiles(smallest, q.radius, gc.X_COLS))
        twin = gc.BY_NAME[case["twin"]]
        tq = next(t for t in gc.case_plan(twin, mode).passes if t.axis == q.axis)
        tn = twin["shape"][0] if tq.transposed else twin["shape"][1]
        assert (tq.radius, tq.transposed, tq.kernel) == (q.radius, q.transposed, q.kernel)
        assert tn == smallest - 1 and not any(any(t.tiles) for t in gc.case_plan(twin, mode).passes)


def test_the_switch_is_on_one_plane():
    a, b = gc.BY_NAME["switch_r63"], gc.BY_NAME["switch_r64"]
    assert a["shape"] == b["shape"] and gc.case_plan(a).ry + 1 == gc.case_plan(b).ry == gc.TRANSPOSE_RADIUS


def test_the_refusals_are_one_radius_past_the_largest():
    for ok, over, axis in (("max_rx", "over_rx", "x"), ("max_ry", "over_ry", "y")):
        a, b = gc.BY_NAME[ok], gc.BY_NAME[over]
        assert a["shape"] == b["shape"]
        pa, pb = gc.case_plan(a), gc.case_plan(b)
        assert pa.refused is None and pb.refused == axis
        assert (pa.rx if axis == "x" else pa.ry) + 1 == (pb.rx if axis == "x" else pb.ry)
    # the direct y pass at those radii only because the transposed route is refused: one column fewer and it is taken
    ny, nx = gc.BY_NAME["max_ry"]["shape"]
    assert nx == 65535 * gc.X_ROWS + 1 and gc.plan(ny, nx - 1, 59.5, 0.0).route_y == "transposed"


def test_the_tap_cache_case_wraps_evicts_and_varies_the_key():
    calls = gc.BY_NAME["tap_cache"]["calls"]
    distinct = list(dict.fromkeys(calls))
    assert len(distinct) > gc.TAP_SLOTS and len(calls[:40]) == len(set(calls[:40])) == 40
    assert calls[40] == calls[0]  # 40 misses later slot 0 .. 7 have been overwritten: the first key is gone
    s = [c for c in calls if c[0] == calls[41][0]]
    assert [t for _, t in s] == [3.0, 4.0, 3.0]
    assert len({gc.radius_of(*c) for c in calls}) > 8


def _nonfinite_set(case, pixel):
    a = gc.nonfinite_input(case, pixel, np.nan)
    return ~np.isfinite(gc.reference(a, case["sy"], case["sx"], case["truncate"]))


@pytest.mark.parametrize("case", gc.cases("nonfinite"), ids=lambda c: c["name"])
def test_nonfinite_cases_leave_a_rim(case):
    ny, nx = case["shape"]
    m = gc.NONFINITE_MARGIN
    for pixel in case["pixels"]:
        bad = _nonfinite_set(case, pixel)
        assert bad.any()
        ys, xs = np.nonzero(bad)
        room = {"top": ys.min(), "bottom": ny - 1 - ys.max(), "left": xs.min(), "right": nx - 1 - xs.max()}
        for edge, free in room.items():
            if edge in pixel["touches"]:
                # the window crosses the reflecting edge: the set reaches it, and is wider than on open ground
                assert free == 0, (pixel, edge)
            else:
                assert free >= m, (pixel, edge, free)
        # scipy's set is the window, +-radius per filtered axis (folded back at an edge it touches)
        p = gc.case_plan(case)
        for r, lo, hi, c0, e0 in ((p.ry or 0, ys.min(), ys.max(), pixel["y"], "top"), (p.rx or 0, xs.min(), xs.max(), pixel["x"], "left")):
            assert hi == c0 + r and lo == (0 if e0 in pixel["touches"] else c0 - r)


def test_nonfinite_positions_cover_what_the_kernels_distinguish():
    xcases = [c for c in gc.cases("nonfinite") if gc.case_plan(c).rx is not None and gc.case_plan(c).ry is None]
    assert {gc.case_plan(c).rx < 16 for c in xcases} == {True, False}
    for c in xcases:
        cols = [p["x"] for p in c["pixels"]]
        assert gc.X_COLS - 1 in cols and gc.X_COLS in cols and {x % 4 for x in cols} == {0, 1, 2, 3}
        assert any("left" in p["touches"] for p in c["pixels"])
    plans = [gc.case_plan(c) for c in gc.cases("nonfinite")]
    assert {(p.route_y, p.do_x) for p in plans} == {("skip", True), ("direct", False), ("direct", True), ("transposed", False), ("transposed", True)}
    direct = [p.ry for p in plans if p.route_y == "direct"]
    assert min(direct) < 16 <= max(direct)
    # through the transposed plane the row is the x pass's column: every residue mod 4, and the reflecting edge
    t = gc.BY_NAME["nf_t_r64"]
    assert {p["y"] % 4 for p in t["pixels"]} == {0, 1, 2, 3} and any("top" in p["touches"] for p in t["pixels"])
    for c in gc.cases("nonfinite"):
        assert c["modes"] == gc.ALL_MODES
