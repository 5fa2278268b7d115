"""CPU tier of maria_amd.flagging: the reference's median against a clamp-and-sort rebuild, the flag
downsampling against a loop, the glitch injector's reproducibility, and the refusals, which come before any device call."""

import flagging_ref as ref
import numpy as np
import pytest
import torch

from maria_amd import flagging


def tied_rows(D, T, seed=0):
    """Noise plus a drift, every seventh sample set to the row's first: ties in every window."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((D, T)) + np.linspace(0.0, 3.0, T) + 5).astype(np.float32)
    x[:, ::7] = x[:, :1]
    return x


@pytest.mark.parametrize("T", [1, 2, 5, 11, 300])
@pytest.mark.parametrize("h", [1, 5, 15])
def test_reference_median_is_clamp_and_sort(T, h):
    x = tied_rows(3, T, seed=T + h)
    r, med = ref.median_residual(x, h)
    np.testing.assert_array_equal(med, ref.median_by_sorting(x, h))
    np.testing.assert_array_equal(r, x - med)
    assert r.dtype == np.float32


def test_reference_sigma_is_the_lower_median():
    x = tied_rows(4, 300, seed=2)  # an even T: numpy's median would average two
    r, _ = ref.median_residual(x, 5)
    want = 1.4826 * torch.median(torch.as_tensor(np.abs(r)), dim=1).values.double().numpy()
    np.testing.assert_array_equal(ref.robust_sigma(x, 5), want)


def test_reference_flags_grow_the_right_way():
    x = np.zeros((1, 40), np.float32)
    x[0, 20] = 10.0
    f, count = ref.flags(x, 2, [1.0], grow_before=2, grow_after=5)
    want = np.zeros(40, np.uint8)
    want[18:20], want[20], want[21:26] = 2, 1, 2
    np.testing.assert_array_equal(f[0], want)
    assert count[0] == 8


@pytest.mark.parametrize("T,q", [(1, 2), (7, 2), (8, 2), (100, 4), (101, 4), (33, 32), (300, 7), (50, 1)])
def test_downsample_flags_against_a_loop(T, q):
    rng = np.random.default_rng(T * q)
    f = (rng.random((5, T)) < 0.03).astype(np.uint8) * rng.integers(1, 3, (5, T)).astype(np.uint8)
    f[0] = 0
    f[1, -1] = 2
    f[2, 0] = 1
    got = flagging.downsample_flags(torch.as_tensor(f), q)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, -(-T // q))
    np.testing.assert_array_equal(got.numpy(), ref.downsample_flags(f, q))
    np.testing.assert_array_equal(flagging.downsample_flags(torch.as_tensor(f), q, chunk_bytes=1).numpy(), got.numpy())


def test_inject_glitches_is_reproducible_by_seed():
    base = torch.as_tensor(tied_rows(6, 500, seed=1))
    a, b, c = base.clone(), base.clone(), base.clone()
    ma = flagging.inject_glitches(a, 3, (50.0, 500.0), 3.0, seed=11)
    mb = flagging.inject_glitches(b, 3, (50.0, 500.0), 3.0, seed=11)
    mc = flagging.inject_glitches(c, 3, (50.0, 500.0), 3.0, seed=12)
    assert torch.equal(a, b) and torch.equal(ma, mb) and not torch.equal(ma, mc)
    assert ma.dtype == torch.bool and bool((ma.sum(dim=1) == 3).all())
    onsets, amps = flagging.draw_glitches(6, 500, 3, (50.0, 500.0), 11)
    assert np.array_equal(np.argwhere(ma.numpy())[:, 1].reshape(6, 3), onsets)
    assert np.all((np.abs(amps) >= 50) & (np.abs(amps) <= 500)) and (amps > 0).any() and (amps < 0).any()
    # one glitch alone: amp * exp(-k / tau) for k < 4 tau, nothing after
    x = torch.zeros((1, 64), dtype=torch.float32)
    m = flagging.inject_glitches(x, 1, 8.0, 2.5, seed=0)
    s = int(np.flatnonzero(m.numpy()[0])[0])
    k = np.arange(64 - s)
    want = np.where(k < 10, np.exp(-k / 2.5), 0.0) * 8.0
    assert np.allclose(np.abs(x.numpy()[0, s:]), want, rtol=1e-6, atol=0) and not x[0, :s].any()


def test_refusals_come_before_any_device_call(monkeypatch):
    """Everything the three entries refuse raises ValueError on the host: no context is made and no entry is called."""
    from maria_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call")

    monkeypatch.setattr(_lib.Context, "__init__", no_device)
    monkeypatch.setattr(_lib.Context, "call", no_device)
    x = torch.zeros((3, 100), dtype=torch.float32)
    f = torch.zeros((3, 100), dtype=torch.uint8)
    shape = {
        "D 0": dict(x=x[:0]),
        "T 0": dict(x=x[:, :0]),
        "1-D x": dict(x=x[0]),
        "float64 x": dict(x=x.double()),
        "numpy x": dict(x=np.zeros((3, 100), np.float32)),
        "strided samples": dict(x=x[:, ::2]),
        "pitch < T": dict(x=torch.as_strided(x, (3, 100), (50, 1))),
        "host x": dict(x=x),  # the last refusal: everything else about this call is in order
    }
    window = {"h 0": dict(x=x, half_window=0), "h 16": dict(x=x, half_window=16), "h 2.5": dict(x=x, half_window=2.5)}
    cases = {
        flagging.median_residual: {
            **shape, **window,
            "out is x": dict(x=x, out=x),
            "out overlaps x": dict(x=x[:2], out=torch.as_strided(x, (2, 100), (100, 1), 50)),
            "out shape": dict(x=x, out=torch.zeros((3, 99))),
            "out dtype": dict(x=x, out=torch.zeros((3, 100), dtype=torch.float64)),
            "out pitch": dict(x=x, out=torch.as_strided(torch.zeros(300), (3, 100), (60, 1))),
        },
        flagging.robust_sigma: {**shape, **window, "no scratch": dict(x=x, scratch_bytes=0)},
        flagging.find_glitches: {
            **shape, **window,
            "grow 65": dict(x=x, grow=(65, 0)),
            "grow -1": dict(x=x, grow=(0, -1)),
            "grow 1.5": dict(x=x, grow=(1.5, 2)),
            "grow scalar": dict(x=x, grow=3),
            "n_sigma nan": dict(x=x, n_sigma=float("nan")),
            "n_sigma inf": dict(x=x, n_sigma=float("inf"), sigma=1.0),
            "n_sigma < 0": dict(x=x, n_sigma=-1.0),
            "sigma nan": dict(x=x, sigma=np.array([1.0, np.nan, 1.0])),
            "sigma inf": dict(x=x, sigma=float("inf")),
            "sigma < 0": dict(x=x, sigma=torch.tensor([1.0, -1.0, 1.0])),
            "sigma shape": dict(x=x, sigma=np.ones(4)),
        },
    }
    for fn, bad in cases.items():
        for name, kw in bad.items():
            with pytest.raises(ValueError):
                fn(**kw)
                pytest.fail(f"{fn.__name__}: {name}")
    fill = {
        **{k: dict(v, flags=f) for k, v in shape.items()},
        "n_fit 0": dict(x=x, flags=f, n_fit=0),
        "n_fit 17": dict(x=x, flags=f, n_fit=17),
        "n_fit 2.5": dict(x=x, flags=f, n_fit=2.5),
        "flags shape": dict(x=x, flags=f[:, :99]),
        "flags dtype": dict(x=x, flags=f.bool()),
        "flags numpy": dict(x=x, flags=f.numpy()),
        "flags strided": dict(x=x, flags=torch.zeros((3, 200), dtype=torch.uint8)[:, ::2]),
        "flags pitch": dict(x=x, flags=torch.as_strided(torch.zeros(300, dtype=torch.uint8), (3, 100), (60, 1))),
    }
    for name, kw in fill.items():
        with pytest.raises(ValueError):
            flagging.gap_fill(**kw)
            pytest.fail(f"gap_fill: {name}")
    for kw in (dict(flags=f.float(), q=2), dict(flags=f[0], q=2), dict(flags=f, q=0), dict(flags=f, q=1.5)):
        with pytest.raises(ValueError):
            flagging.downsample_flags(**kw)
    for kw in (dict(n_per_row=101, amplitude=1.0, tau_samples=3, seed=0), dict(n_per_row=1, amplitude=-1.0, tau_samples=3, seed=0),
               dict(n_per_row=1, amplitude=(2.0, 1.0), tau_samples=3, seed=0), dict(n_per_row=1, amplitude=1.0, tau_samples=0, seed=0)):
        with pytest.raises(ValueError):
            flagging.inject_glitches(x, **kw)
    assert not x.any()


def test_tod_flags_default_to_none():
    from maria_amd.sim import TOD

    tod = TOD({"a": np.zeros((2, 3), np.float32)}, dets=None, coords=None)
    assert tod.flags is None
    f = torch.zeros((2, 3), dtype=torch.uint8)
    assert TOD({"a": np.zeros((2, 3), np.float32)}, None, None, "K_RJ", {}, f).flags is f
    tod._calibrator = lambda data, to_krj: data
    tod.flags = f
    assert tod.to("K_RJ").flags is f
