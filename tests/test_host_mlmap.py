"""MaximumLikelihoodMapper's argument checks and the map-maker's C entry points (no GPU needed)."""

import numpy as np
import pytest


def _tod(n=6, T=50, units="K_RJ"):
    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    dets = Detectors(np.zeros((n, 2)), [Band(center=150e9, width=30e9, name="f150")])
    t = np.arange(T) / 50.0
    return TOD({"map": np.zeros((n, T), np.float32)}, dets, Coordinates(t, np.zeros(T), np.full(T, 1.0), offsets=dets.offsets), units=units)


def test_ml_mapper_argument_checks():
    from maria_amd.mappers import MaximumLikelihoodMapper

    tod = _tod()
    m = MaximumLikelihoodMapper([tod], center=(10.0, 20.0), width=1.0, resolution=0.1, frame="az/el")
    assert (m.n_eta, m.n_xi) == (10, 10) and m.stokes == "IQU" and not m.bilinear and m.noise_weights == "inverse_variance"
    assert (m.max_iter, m.tol, m.rcond) == (100, 1e-6, 1e-3)
    with pytest.raises(RuntimeError):
        _ = m.map
    with pytest.raises(NotImplementedError):
        MaximumLikelihoodMapper([tod], center=(0, 0), width=1.0, resolution=0.1, frame="galactic")
    with pytest.raises(ValueError, match="K_RJ"):
        MaximumLikelihoodMapper([_tod(units="pW")], center=(0, 0), width=1.0, resolution=0.1)
    with pytest.raises(ValueError, match="resolution"):
        MaximumLikelihoodMapper([tod], center=(0, 0), width=1.0)
    with pytest.raises(ValueError, match="noise_weights"):
        MaximumLikelihoodMapper([tod], center=(0, 0), width=1.0, resolution=0.1, noise_weights=np.ones(5))
    with pytest.raises(ValueError, match="noise_weights"):
        MaximumLikelihoodMapper([tod], center=(0, 0), width=1.0, resolution=0.1, noise_weights="white")
    with pytest.raises(ValueError, match="stokes"):
        MaximumLikelihoodMapper([tod], center=(0, 0), width=1.0, resolution=0.1, stokes="IQUV")
    ok = MaximumLikelihoodMapper([tod], center=(0, 0), width=1.0, resolution=0.1, noise_weights=np.ones(6), stokes="I", bilinear=True)
    assert ok.bilinear and ok.stokes == "I"


def test_ml_symbols_are_exported_and_bound():
    import ctypes as C

    from maria_amd import _lib

    lib = _lib.load()
    for name in ("mrx_map_project", "mrx_map_normal_work_bytes", "mrx_map_normal_apply", "mrx_bin_map_blocks", "mrx_map_block_solve"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the work-buffer query needs no device: the routed form's buffer for a small map, none for a map of > 2048 regions
    small = _lib.MrxSkyMap(None, 1, 3, 64, 128, 1.0, -0.01, -1.0, 0.01, 0.0, 0.5, 0, 0)
    lo, full = C.c_size_t(), C.c_size_t()
    assert lib.mrx_map_normal_work_bytes(C.byref(small), 100, 5000, C.byref(lo), C.byref(full)) == 0
    assert 0 < lo.value and full.value == 5 * lo.value  # ceil(5000 / 1024) columns of tiles
    big = _lib.MrxSkyMap(None, 2, 3, 4096, 4096, 1.0, -1e-4, -1.0, 1e-4, 0.0, 0.5, 0, 0)
    assert lib.mrx_map_normal_work_bytes(C.byref(big), 100, 5000, C.byref(lo), C.byref(full)) == 0 and lo.value == full.value == 0
