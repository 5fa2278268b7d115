"""DestripingMapper's argument checks and the destriper's C entry points (no GPU needed)."""

import numpy as np
import pytest
from test_host_mlmap import _tod


def test_destriping_mapper_argument_checks():
    from maria_amd.mappers import DestripingMapper

    tod = _tod(T=500)  # 50 Hz
    kw = dict(center=(0, 0), width=1.0, resolution=0.1)
    m = DestripingMapper([tod], frame="az/el", **kw)
    assert m.baseline_length == 1.0 and m.baseline_samples == [50] and m.stokes == "IQU" and m.noise_weights == "inverse_variance"
    assert (m.max_iter, m.tol, m.rcond) == (100, 1e-6, 1e-3)
    assert DestripingMapper([tod], baseline_length=0.32, **kw).baseline_samples == [16]
    assert DestripingMapper([tod], baseline_length=100.0, **kw).baseline_samples == [5000]  # longer than the TOD: one baseline
    with pytest.raises(RuntimeError):
        _ = m.map
    with pytest.raises(ValueError, match="at least 16"):
        DestripingMapper([tod], baseline_length=0.3, **kw)  # 15 samples
    with pytest.raises(NotImplementedError, match="nearest"):
        DestripingMapper([tod], bilinear=True, **kw)
    with pytest.raises(ValueError, match="stokes"):
        DestripingMapper([tod], stokes="IQUV", **kw)
    with pytest.raises(ValueError, match="stokes"):
        DestripingMapper([tod], stokes="QQ", **kw)
    with pytest.raises(ValueError, match="noise_weights"):
        DestripingMapper([tod], noise_weights=np.ones(5), **kw)
    with pytest.raises(ValueError, match="noise_weights"):
        DestripingMapper([tod], noise_weights="white", **kw)
    with pytest.raises(ValueError, match="K_RJ"):
        DestripingMapper([_tod(units="pW")], **kw)
    ok = DestripingMapper([tod], noise_weights=np.ones(6), stokes="QU", baseline_length=0.5, **kw)
    assert ok.stokes == "QU" and ok.baseline_samples == [25]


def test_destriper_symbols_are_exported_and_bound():
    import ctypes as C

    from maria_amd import _lib

    lib = _lib.load()
    for name in ("mrx_baseline_reduce", "mrx_bin_map_baselines"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # mrx_map_normal_work_bytes sizes mrx_bin_map_baselines' buffer; it needs no device
    small = _lib.MrxSkyMap(None, 1, 3, 64, 128, 1.0, -0.01, -1.0, 0.01, 0.0, 0.5, 0, 0)
    lo, full = C.c_size_t(), C.c_size_t()
    assert lib.mrx_map_normal_work_bytes(C.byref(small), 37, 3301, C.byref(lo), C.byref(full)) == 0
    assert 0 < lo.value and full.value == 4 * lo.value  # ceil(3301 / 1024) columns of tiles
