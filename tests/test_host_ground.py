"""CPU tier of maria_amd.ground: the azimuth binning and the bin lists against loops, the reference against a
brute-force double loop, the host-side helpers, and the refusals, which come before any device call."""

import ground_ref as ref
import numpy as np
import pytest
import torch

from maria_amd import ground


def scans():
    t = np.arange(700) / 50.0
    return {
        "plain": np.radians(120.0 + 3.0 * np.sin(2 * np.pi * t / 7.0)),
        "across 0 / 2 pi": np.radians(1.0 + 4.0 * np.sin(2 * np.pi * t / 5.0)) % (2 * np.pi),
        "near pi": np.radians(179.0 + 2.0 * np.cos(2 * np.pi * t / 3.0)),
        "negative": np.radians(-40.0 + 10.0 * np.sin(2 * np.pi * t / 9.0)),
    }


@pytest.mark.parametrize("n_bins", [1, 2, 32, 360])
@pytest.mark.parametrize("name", list(scans()))
def test_azimuth_bins_against_a_loop(name, n_bins):
    az = scans()[name]
    bins, lo, hi = ground.azimuth_bins(az, n_bins)
    want, lo_w, hi_w = ref.azimuth_bins_by_loop(az, n_bins)
    assert bins.dtype == np.int32 and bins.shape == az.shape and (lo, hi) == (lo_w, hi_w)
    np.testing.assert_array_equal(bins, want)
    assert bins.min() == 0 and bins.max() == n_bins - 1
    # one interval, as wide as the scan: a scan across 0 / 2 pi is not split into two ends of the circle
    assert hi - lo < np.radians(21.0)
    assert bins[np.argmax((az - lo + np.pi) % (2 * np.pi))] == n_bins - 1  # the top edge belongs to the last bin


def test_azimuth_bins_of_a_stare_and_of_a_given_interval():
    bins, lo, hi = ground.azimuth_bins(np.full(50, 2.5), 16)
    assert lo == hi == 2.5 and not bins.any() and bins.dtype == np.int32
    az = scans()["across 0 / 2 pi"]
    _, lo0, hi0 = ground.azimuth_bins(az, 8)
    lo, hi = lo0 + 0.25 * (hi0 - lo0), hi0 - 0.25 * (hi0 - lo0)
    bins, lo_r, hi_r = ground.azimuth_bins(az, 8, lo=lo, hi=hi)
    want, _, _ = ref.azimuth_bins_by_loop(az, 8, lo=lo, hi=hi)
    np.testing.assert_array_equal(bins, want)
    assert (lo_r, hi_r) == (lo, hi) and (bins == -1).sum() > 100 and (bins >= 0).sum() > 100 and bins.max() == 7
    for kw in (dict(n_bins=0), dict(n_bins=ground.MAX_BINS + 1), dict(n_bins=2.5), dict(n_bins=4, lo=1.0, hi=0.5),
               dict(n_bins=4, lo=float("nan"))):
        with pytest.raises(ValueError):
            ground.azimuth_bins(az, **kw)
    with pytest.raises(ValueError):
        ground.azimuth_bins(az[:, None], 4)


@pytest.mark.parametrize("T,n_bins", [(1, 1), (1, 5), (40, 3), (300, 7), (300, 400)])
def test_bin_lists_against_a_loop(T, n_bins):
    rng = np.random.default_rng(T + n_bins)
    bins = rng.integers(-1, n_bins, T).astype(np.int32)
    if n_bins > 2:
        bins[bins == 1] = 2  # an empty bin between occupied ones
    order, start = ground.bin_lists(bins, n_bins)
    want_order, want_start = ref.bin_lists_by_loop(bins, n_bins)
    assert order.dtype == np.int32 and start.dtype == np.int32 and start.shape == (n_bins + 1,)
    np.testing.assert_array_equal(order, want_order)
    np.testing.assert_array_equal(start, want_start)
    assert start[0] == 0 and start[-1] == order.size == (bins >= 0).sum() and np.all(np.diff(start) >= 0)
    for k in range(n_bins):  # stable: ascending within a bin
        assert np.all(np.diff(order[start[k]:start[k + 1]]) > 0)
    none, start = ground.bin_lists(np.full(T, -1, np.int32), n_bins)
    assert none.size == 0 and not start.any()
    same, _ = ground.bin_lists(torch.as_tensor(bins), n_bins)  # a tensor key
    np.testing.assert_array_equal(same, order)


def test_reference_against_a_double_loop():
    rng = np.random.default_rng(3)
    D, T, K = 4, 150, 6
    x = rng.standard_normal((D, T)).astype(np.float32)
    model = rng.standard_normal((D, T)).astype(np.float32)
    flags = (rng.random((D, T)) < 0.1).astype(np.uint8) * 2
    bins = rng.integers(-1, K, T)
    bins[bins == 4] = 3  # an empty bin
    flags[2, bins == 0] = 1  # a bin with every sample flagged in one row
    for kw in (dict(), dict(flags=flags), dict(model=model), dict(flags=flags, model=model, min_hits=8)):
        sums, hits, template, absum = ref.bin_reduce(x, bins, K, **kw)
        s2, h2, t2 = ref.bin_reduce_by_loops(x, bins, K, **kw)
        np.testing.assert_allclose(sums, s2, rtol=0, atol=1e-13)
        np.testing.assert_array_equal(hits, h2)
        np.testing.assert_allclose(template, t2, rtol=2.0**-23, atol=1e-13)
        assert not hits[:, 4].any() and not template[:, 4].any() and np.all(absum >= np.abs(sums) - 1e-13)
    assert hits[2, 0] == 0 and np.array_equal(template == 0, hits < 8)
    tpl = rng.standard_normal((D, K)).astype(np.float32)
    for sign in (-1, 1):
        y = ref.bin_apply(x, bins, tpl, sign)
        for d in range(D):
            for t in range(T):
                want = x[d, t] if bins[t] < 0 else (x[d, t] - tpl[d, bins[t]] if sign < 0 else x[d, t] + tpl[d, bins[t]])
                assert y[d, t] == np.float32(want)


def test_shared_template_and_synthetic_ground():
    rng = np.random.default_rng(4)
    sums = torch.as_tensor(rng.standard_normal((5, 7)))
    hits = torch.as_tensor(rng.integers(0, 4, (5, 7)))
    hits[:, 2] = 0
    got = ground.shared_template(sums, hits, min_hits=6)
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 7) and got.is_contiguous()
    n = hits.numpy().sum(axis=0)
    want = np.where(n >= 6, sums.numpy().sum(axis=0) / np.maximum(n, 1), 0.0).astype(np.float32)
    assert (n >= 6).any() and (n < 6).any()
    np.testing.assert_array_equal(got.numpy(), np.broadcast_to(want, (5, 7)))
    assert not ground.shared_template(sums, hits, min_hits=0)[:, 2].any()  # no hits: 0 and not a division by zero
    with pytest.raises(ValueError):
        ground.shared_template(sums, hits[:, :6])
    g = ground.synthetic_ground(10, 32, 0.05, seed=3)
    assert g.dtype == np.float32 and g.shape == (10, 32)
    phase = np.random.default_rng(3).uniform(0.0, 2 * np.pi)
    want = 0.05 * (1 + 0.1 * np.arange(10)[:, None] / 10) * np.cos(2 * np.pi * np.arange(32)[None, :] / 32 + phase)
    np.testing.assert_allclose(g, want, rtol=0, atol=2.0**-24 * 0.06)
    np.testing.assert_array_equal(g, ground.synthetic_ground(10, 32, 0.05, seed=3))
    assert not np.array_equal(g, ground.synthetic_ground(10, 32, 0.05, seed=4))


def test_refusals_come_before_any_device_call(monkeypatch):
    """Everything the two entries refuse raises ValueError on the host: no context is made and no entry is called."""
    from maria_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call")

    monkeypatch.setattr(_lib.Context, "__init__", no_device)
    monkeypatch.setattr(_lib.Context, "call", no_device)
    x = torch.zeros((3, 100), dtype=torch.float32)
    f = torch.zeros((3, 100), dtype=torch.uint8)
    b = np.zeros(100, np.int32)
    tpl = torch.zeros((3, 4), dtype=torch.float32)
    shape = {
        "D 0": dict(x=x[:0]),
        "T 0": dict(x=x[:, :0], bins=b[:0]),
        "1-D x": dict(x=x[0]),
        "float64 x": dict(x=x.double()),
        "numpy x": dict(x=np.zeros((3, 100), np.float32)),
        "strided samples": dict(x=x[:, ::2], bins=b[:50]),
        "pitch < T": dict(x=torch.as_strided(x, (3, 100), (50, 1))),
        "bins length": dict(x=x, bins=b[:99]),
        "bins 2-D": dict(x=x, bins=b[None, :]),
        "bins float": dict(x=x, bins=b.astype(np.float32)),
        "bins -2": dict(x=x, bins=np.where(np.arange(100) == 5, -2, 0)),
        "bins n_bins": dict(x=x, bins=np.where(np.arange(100) == 5, 4, 0)),
        "host x": dict(x=x),  # the last refusal: everything else about this call is in order
    }
    reduce = {
        **shape,
        "n_bins 0": dict(x=x, n_bins=0),
        "n_bins 4097": dict(x=x, n_bins=ground.MAX_BINS + 1),
        "n_bins 2.5": dict(x=x, n_bins=2.5),
        "min_hits -1": dict(x=x, min_hits=-1),
        "min_hits 1.5": dict(x=x, min_hits=1.5),
        "flags shape": dict(x=x, flags=f[:, :99]),
        "flags dtype": dict(x=x, flags=f.bool()),
        "flags numpy": dict(x=x, flags=f.numpy()),
        "flags pitch": dict(x=x, flags=torch.as_strided(torch.zeros(300, dtype=torch.uint8), (3, 100), (60, 1))),
        "model shape": dict(x=x, model=x[:2]),
        "model dtype": dict(x=x, model=x.double()),
        "model numpy": dict(x=x, model=x.numpy()),
        "model strided": dict(x=x, model=torch.zeros((3, 200))[:, ::2]),
    }
    for name, kw in reduce.items():
        kw = {"bins": b, "n_bins": 4, **kw}
        with pytest.raises(ValueError):
            ground.bin_template(**kw)
            pytest.fail(f"bin_template: {name}")
    apply = {
        **shape,
        "sign 0": dict(x=x, sign=0),
        "sign 2": dict(x=x, sign=2),
        "template rows": dict(x=x, template=tpl[:2]),
        "template dtype": dict(x=x, template=tpl.double()),
        "template numpy": dict(x=x, template=tpl.numpy()),
        "template strided": dict(x=x, template=torch.zeros((3, 8))[:, ::2]),
        "template K 0": dict(x=x, template=tpl[:, :0]),
        "template K 4097": dict(x=x, template=torch.zeros((3, ground.MAX_BINS + 1))),
        "out shape": dict(x=x, out=torch.zeros((3, 99))),
        "out dtype": dict(x=x, out=torch.zeros((3, 100), dtype=torch.float64)),
        "out pitch": dict(x=x, out=torch.as_strided(torch.zeros(300), (3, 100), (60, 1))),
        "out overlaps x": dict(x=x[:2], out=torch.as_strided(x, (2, 100), (100, 1), 50)),
    }
    for name, kw in apply.items():
        kw = {"bins": b, "template": tpl, **kw}
        with pytest.raises(ValueError):
            ground.apply_template(**kw)
            pytest.fail(f"apply_template: {name}")
    for kw in (dict(bins=b, n_bins=0), dict(bins=np.full(10, 4), n_bins=4), dict(bins=np.full(10, -2), n_bins=4)):
        with pytest.raises(ValueError):
            ground.bin_lists(**kw)
    for kw in (dict(D=0, n_bins=4), dict(D=3, n_bins=0)):
        with pytest.raises(ValueError):
            ground.synthetic_ground(amplitude=1.0, seed=0, **kw)


def test_remove_ground_refuses_on_the_host(monkeypatch):
    from maria_amd import _lib
    from maria_amd.sim import TOD, Coordinates

    def no_device(*a, **k):
        raise AssertionError("a device call")

    monkeypatch.setattr(_lib.Context, "__init__", no_device)
    t = np.arange(20) / 10.0
    tod = TOD({"a": np.zeros((2, 20), np.float32)}, None, Coordinates(t, np.linspace(0.1, 0.2, 20), np.full(20, 1.0)))
    for kw in (dict(n_bins=0), dict(n_bins=ground.MAX_BINS + 1), dict(bins=np.zeros(19, np.int32)), dict(n_bins=4, bins=np.full(20, 4)),
               dict(min_hits=-1), dict(into="b")):
        with pytest.raises(ValueError):
            tod.remove_ground(**kw)
