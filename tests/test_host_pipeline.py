"""CPU tests of maria_amd.pipeline_host: the host geometry that decides which kernel form a DevicePath run takes,
against the rule written out here and against values recorded from the methods these functions were moved out of."""

import os

import numpy as np
import pytest

from helpers import small_problem
from maria_amd import pipeline_host as ph
from maria_amd import synthetic
from test_gpu_calibration import _cal_tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_f32_cell_is_the_rule_written_out():
    """f32_cell against jax's float32 cell rule: 200 random axes of 2 to 40 nodes, x inside, exactly on a node, on the
    first and the last node and outside both ends; index, weight and off-axis flag exactly."""
    rng = np.random.default_rng(2024)
    for _ in range(200):
        n = int(rng.integers(2, 41))
        axis = np.cumsum(rng.uniform(0.01, 3.0, n)) + rng.uniform(-50.0, 300.0)
        g = axis.astype(np.float32)
        xs = [rng.uniform(axis[0], axis[-1]), rng.uniform(axis[0], axis[-1]), float(g[rng.integers(0, n)]), float(g[0]), float(g[-1]),
              axis[0] - rng.uniform(1e-3, 5.0), axis[-1] + rng.uniform(1e-3, 5.0)]
        for x in xs:
            xf = np.float32(x)
            i = int(np.clip(np.searchsorted(g, xf, "left") - 1, 0, n - 2))
            w = np.float32((xf - g[i]) / (g[i + 1] - g[i]))
            oob = bool(xf < g[0] or xf > g[-1])
            gi, gw, goob = ph.f32_cell(axis, x)
            assert (gi, goob) == (i, oob) and type(goob) is bool
            assert gw.dtype == np.float32 and gw == w


@pytest.fixture(scope="module")
def cal():
    """The input of test_gpu_calibration.py::test_coarse_krj_form_stays_within_its_bound, collapsed once."""
    p = small_problem(n_det=300, n_bands=2, n_layers=2, gain=True)
    _, el_full = synthetic.daisy_scan(p["t"])
    roll = np.radians(17.0)
    R = np.array([[np.cos(roll), -np.sin(roll)], [np.sin(roll), np.cos(roll)]])
    radius = float(np.hypot(*(p["offsets"] @ R.T).T).max())  # (of the whole focal plane, as set_calibration forms it)
    tables = _cal_tables(2)
    el_axis, dens = ph.collapse_calibration(tables, 273.15, 1.0, [False, True])
    return dict(p=p, tables=tables, el_axis=el_axis, dens=dens, radius=radius)


def test_calibration_collapse_and_bound(cal):
    """The collapsed denominators bit for bit, the coarse-form bound to 1e-12 and the K_RJ split exactly as
    DevicePath.set_calibration / coarse_krj_bound / _krj_split gave them before the move."""
    p = cal["p"]
    assert np.array_equal(cal["el_axis"], cal["tables"][0]["el"])
    want = np.load(os.path.join(GOLDEN, "host_pipeline_dens.npy"))
    assert cal["dens"].dtype == np.float32 and want.dtype == np.float32
    assert cal["dens"].tobytes() == want.tobytes()
    assert cal["radius"] == 0.004363323129985824
    bound = ph.coarse_krj_bound(cal["el_axis"], cal["dens"], cal["radius"], p["el_a"], p["t"], p["ta"])
    assert bound == pytest.approx(1.441880963938568e-06, rel=1e-12)
    assert 0 < bound <= ph.COARSE_KRJ_LIMIT == 4e-6
    assert (len(p["t"]), len(p["ta"])) == (1000, 200)
    assert ph.krj_split(p["t"], p["ta"], len(p["t"])) == 995


def test_coarse_form_refusals(cal):
    """The three refusals of the GPU test: a table whose axis the focal plane may leave, the zenith, a 1 deg per knot slew."""
    p = cal["p"]
    low = [dict(t, el=np.radians(np.linspace(59.5, 90.1, 33))) for t in cal["tables"]]
    el_axis, dens = ph.collapse_calibration(low, 273.15, 1.0, [False, True])
    assert ph.coarse_krj_bound(el_axis, dens, cal["radius"], p["el_a"], p["t"], p["ta"]) == float("inf")
    Ta = len(p["ta"])
    bound = lambda el_a: ph.coarse_krj_bound(cal["el_axis"], cal["dens"], cal["radius"], el_a, p["t"], p["ta"])  # noqa: E731
    assert bound(np.radians(np.linspace(80.0, 84.0, Ta))) == float("inf")
    slew = bound(np.radians(np.linspace(20.0, 20.0 + 1.0 * Ta, Ta) % 60 + 15))
    assert slew > ph.COARSE_KRJ_LIMIT and slew == pytest.approx(0.1296513419830586, rel=1e-12)


def test_sampled_margins_px():
    """The margins of the whole focal plane (the function takes the whole problem: no shard can change them)."""
    got = ph.sampled_margins_px(small_problem(n_det=700, n_bands=2, n_layers=3))
    want = [(43.254592036223556, 62.77401411425819), (38.46317187988002, 61.28001576088743), (33.61300035814365, 59.705935478025914)]
    assert len(got) == 3
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=1e-12, atol=0)
