"""The one field upload of the ``TOD`` methods (maria_amd.tod) on the device: whatever form a field comes
in -- a float64 host array, rows of a wider device buffer (a padded row pitch), the transpose of a device tensor -- every
method gives, bit for bit, what it gives on contiguous float32 device tensors of the same values, and leaves its input alone.

D = 3 rows of T = 1030 samples: one full tile of 1024 samples and a partial second one.  The padded field's row pitch is
1032, and its pad (two samples a row and a whole fourth row) holds NaN."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, T = 3, 1030
DEV = "cuda:0"


def bits(x):
    import torch

    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64 if x.dtype == torch.float64 else x.dtype)


def same(a, b, where="result"):
    """Bit equality of two results of any shape: tensors, arrays, numbers, and dicts, lists and tuples of them."""
    import torch

    assert type(a) is type(b), where
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)), where
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            same(u, v, f"{where}[{i}]")
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), where
    else:
        assert a == b, where


def same_tod(a, b, where):
    same(a.data, b.data, f"{where}.data")
    same(a.flags, b.flags, f"{where}.flags")
    same(a.metadata, b.metadata, f"{where}.metadata")
    same(a.coords.t, b.coords.t, f"{where}.coords.t")
    assert a.units == b.units, where


@pytest.fixture(scope="module")
def tods():
    """(mixed, plain, buffers): the TOD of the three kinds of fields, the same on contiguous float32 device tensors, and
    the device buffers behind the mixed one's fields."""
    import torch

    from maria_amd.instrument import Band, Detectors
    from maria_amd.sim import TOD, Coordinates

    rng = np.random.default_rng(33)
    a = rng.standard_normal((D, T)) + 1e-3 * np.arange(T)[None, :]  # float64 on the host, with a drift
    a[1, 300] += 40.0  # a glitch
    a[2, 600:] += 12.0  # a jump
    padded = torch.full((4, 1032), float("nan"), dtype=torch.float32, device=DEV)
    padded[:D, :T] = torch.as_tensor(rng.standard_normal((D, T)).astype(np.float32))
    b = padded[:D, :T]
    wide = torch.as_tensor(rng.standard_normal((T, D)).astype(np.float32)).to(DEV)
    c = wide.t()
    assert b.stride() == (1032, 1) and c.stride() == (1, D)
    t = np.arange(T) / 50.0
    phase = (np.arange(T) % 400) / 200.0  # a triangle wave of 400 samples: turnarounds at 200, 400, 600, 800 and 1000
    az = 0.5 + 0.02 * np.where(phase < 1.0, phase, 2.0 - phase)
    coords = Coordinates(t, az, np.full(T, 1.0), offsets=np.zeros((D, 2)))
    dets = Detectors(np.zeros((D, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int))
    flags = torch.as_tensor((rng.random((D, T)) < 0.03).astype(np.uint8)).to(DEV)
    assert 0.01 < float(flags.float().mean()) < 0.06
    mixed = TOD({"a": a, "b": b, "c": c}, dets=dets, coords=coords, metadata={"site": "here"}, flags=flags)
    plain = TOD({k: torch.as_tensor(v).to(DEV, torch.float32).contiguous() for k, v in mixed.data.items()}, dets=dets, coords=coords,
                metadata={"site": "here"}, flags=flags.clone())
    return mixed, plain, {"a": a, "padded": padded, "wide": wide, "flags": flags}


def _calls():
    from maria_amd import regress

    return {
        "psd": lambda tod: tod.psd(device=DEV),
        "psd of one field": lambda tod: tod.psd(field="b", device=DEV),
        "downsample": lambda tod: tod.downsample(2, device=DEV),
        "flag_glitches": lambda tod: tod.flag_glitches(device=DEV),
        "fix_jumps": lambda tod: tod.fix_jumps(device=DEV),
        "remove_ground": lambda tod: tod.remove_ground(device=DEV),
        "regress": lambda tod: tod.regress(regress.legendre_templates(T, 1), device=DEV),
        "remove_common_mode": lambda tod: tod.remove_common_mode(groups=None, device=DEV),
        "filter_subscans": lambda tod: tod.filter_subscans(device=DEV),
        "deconvolve_time_constants": lambda tod: tod.deconvolve_time_constants(tau=0.01, device=DEV),
        "stats": lambda tod: tod.stats(device=DEV),
        "cut": lambda tod: tod.cut(device=DEV),
    }


@pytest.mark.parametrize("name", list(_calls()))
def test_a_method_gives_the_bits_of_contiguous_fields(tods, name):
    import torch

    from maria_amd.sim import TOD

    mixed, plain, buffers = tods
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v.clone()) for k, v in buffers.items()}
    call = _calls()[name]
    got, want = call(mixed), call(plain)
    torch.cuda.synchronize()
    if isinstance(got, TOD):
        same_tod(got, want, name)
        assert name in ("downsample",) or (got.dets is mixed.dets and got.coords is mixed.coords)
        for x in got.data.values():
            assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous()
    else:
        same(got, want, name)
    same(buffers, before, "the input")  # the fields, the pad around them and the flags are as they were
    assert mixed.data["b"].data_ptr() == buffers["padded"].data_ptr() and mixed.data["c"].data_ptr() == buffers["wide"].data_ptr()


def test_downsample_does_not_read_the_pad(tods):
    """The padded field goes to the kernel at its own row pitch: NaN in the pad or zeros, the result is the same."""
    import torch

    from maria_amd.sim import TOD

    mixed, _, buffers = tods
    zeroed = torch.zeros_like(buffers["padded"])
    zeroed[:D, :T] = buffers["padded"][:D, :T]
    other = TOD(dict(mixed.data, b=zeroed[:D, :T]), dets=mixed.dets, coords=mixed.coords, metadata=dict(mixed.metadata), flags=mixed.flags)
    got, want = mixed.downsample(2, device=DEV), other.downsample(2, device=DEV)
    same_tod(got, want, "downsample")
    assert all(bool(torch.isfinite(x).all()) for x in got.data.values())


def test_stats_keeps_no_copy_of_the_fields(tods):
    """``stats`` sums the fields and keeps nothing else: its peak of device memory lies below that of the full upload,
    ``_device_fields``, which holds a float32 copy of every field beside the sum."""
    import torch

    mixed, _, _ = tods

    def peak(call):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        start = torch.cuda.memory_allocated(DEV)
        out = call()
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated(DEV) - start
        del out
        return top

    peak(lambda: mixed.stats(bounds=None, device=DEV))  # (the first call loads what later ones find loaded)
    full = peak(lambda: mixed._device_fields(None, None, None, DEV))
    lean = peak(lambda: mixed.stats(bounds=None, device=DEV))
    print(f"peak device memory: _device_fields {full} bytes, stats {lean} bytes")
    assert lean < full
