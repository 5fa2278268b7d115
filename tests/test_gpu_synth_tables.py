"""GPU tests of where the one-launch synthesis (mrx_atm_synthesize) keeps its band tables: a workgroup stages them (and
the K_RJ cell table) for the first sampler item after entry or after a writer tile -- the tile's images lie over them --
and the items that follow find them in LDS; staging is one round of 16-byte loads plus the last floats singly.

The bar is the one of tests/test_gpu_synthesize.py: every word equal to the two-call form's, on one path whose data
change between launches (`_Alternating`), so that a table left over, half staged or overwritten is a wrong word.  Shape:
300 rows (256 + 44: two detector groups), 256 coarse steps, 10 240 samples (ten time tiles at a ratio of 40), 2 layers --
a few hundred tiles and a few dozen items, so that every resident workgroup alternates between the two roles."""

import numpy as np
import pytest

from helpers import small_problem
from maria_amd import synthetic
from test_gpu_synthesize import _Alternating, _path

pytestmark = pytest.mark.gpu


def _problem(n_bands=1, n_pwv=32, n_el=32, **kw):
    p = small_problem(n_det=300, n_layers=2, n_bands=n_bands, fs=400.0, duration=25.6, gain=True, **kw)
    p["tables"] = synthetic.emission_tables(n_bands, n_pwv, n_el)
    return p


def _launches(path, alt, settings, krj=False):
    """One launch per (sampler_wgs_per_cu, chunk) setting, the two data sets in turn, each held to its reference."""
    import torch

    got = torch.empty_like(alt.want[0])
    for rep, (samplers, chunk) in enumerate(settings):
        v = rep % 2
        alt.select(v)
        got.fill_(float("nan"))
        path.synthesize(got, sampler_wgs_per_cu=samplers, chunk=chunk, krj=krj)
        alt.check(v, got, (samplers, chunk))
        assert path.check_flags() == 0


@pytest.fixture(scope="module")
def base(gpu_ctx):
    """One band, the 32 x 32 table of the benchmark (2 112 floats, in LDS): the path and its two references."""
    path = _path(_problem(), gpu_ctx)
    path.clear_flags()
    assert (path.D, path.Ta, path.T) == (300, 256, 10240)
    return path, _Alternating(path)


@pytest.mark.parametrize(
    "n_bands,n_pwv,n_el",
    [
        (1, 5, 7),     # 82 floats: two past the last whole float4
        (3, 12, 9),    # three bands in LDS, 711 floats: three past
        (3, 32, 32),   # 6 336 floats: no room under the writer's images beside the anchors -- read from global memory
        (1, 80, 80),   # 12 960 floats: above the sampler's own limit for LDS tables
    ],
)
def test_table_sizes_and_bands(gpu_ctx, n_bands, n_pwv, n_el):
    path = _path(_problem(n_bands, n_pwv, n_el), gpu_ctx)
    path.clear_flags()
    _launches(path, _Alternating(path), ((2, 32), (8, 8), (2, 8), (8, 32)))


def test_krj_cell_table_follows_the_band_tables(gpu_ctx):
    """K_RJ on the coarse grid: the sampler's epilogue reads the cell table that is staged with the band tables."""
    from test_gpu_calibration import _cal_tables

    p = _problem(n_bands=2)
    _, el_full = synthetic.daisy_scan(p["t"])
    path = _path(p, gpu_ctx)
    path.clear_flags()
    path.set_calibration(_cal_tables(2), 273.15, 1.0, el_full, p["offsets"], [False, True])
    assert 0 < path.coarse_krj_bound() <= path.COARSE_KRJ_LIMIT
    _launches(path, _Alternating(path, krj=True), ((2, 32), (8, 8), (2, 8), (8, 32)), krj=True)


def test_nobody_dedicated(gpu_ctx, base):
    """MRX_OPT_SAMPLE_WGS_PER_CU = 8: every workgroup alternates tile and item, so the tables come back after every tile."""
    path, alt = base
    _launches(path, alt, ((8, 32), (8, 32), (8, 16), (8, 16)))


@pytest.mark.parametrize("per_cu", [1, 5])
def test_two_dedicated_per_cu(gpu_ctx, base, per_cu):
    """Two dedicated samplers per CU beside one resident workgroup per CU (all but one workgroup sample item after item:
    the tables are staged once) and beside five."""
    from maria_amd import _lib

    path, alt = base
    gpu_ctx.set_option(_lib.OPT_SYNTH_WGS_PER_CU, per_cu)
    try:
        _launches(path, alt, ((2, 32), (2, 32), (2, 16), (2, 16)))
    finally:
        gpu_ctx.set_option(_lib.OPT_SYNTH_WGS_PER_CU, 0)


@pytest.mark.parametrize("chunk", [1, 8, 32])
def test_chunks(gpu_ctx, base, chunk):
    path, alt = base
    _launches(path, alt, ((2, chunk), (8, chunk), (0, chunk), (3, chunk)))


def test_writer_general_in_the_one_launch(gpu_ctx, base):
    """MRX_OPT_WRITER_GENERAL 0 against 1 in the launch's writer role: both equal the two-call form (written with 0)."""
    from maria_amd import _lib

    path, alt = base
    try:
        for general in (0, 1, 0, 1):
            gpu_ctx.set_option(_lib.OPT_WRITER_GENERAL, general)
            _launches(path, alt, ((2, 32), (8, 16)))
    finally:
        gpu_ctx.set_option(_lib.OPT_WRITER_GENERAL, 0)
