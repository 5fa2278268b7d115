"""``maria_amd.tod`` on host tensors: the one field upload in its layers, the order of ``_device_fields``'s
refusals, the derived-TOD rule and the small argument rules of the ``TOD`` methods.  Everything runs on CPU tensors with
``device="cpu"`` and a stand-in for the context: with a context given, the upload touches no device."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from maria_amd.instrument import Band, Detectors
from maria_amd.sim import TOD, Coordinates

D, T = 3, 40
CTX = object()  # never called: the methods refuse, or stop at "must be a device tensor", before they use it
LAST = "must be a device tensor"


def bits(x):
    return x.contiguous().view(torch.int32)


def make_tod(T_fields=T, flags=None, metadata=None):
    """Three fields of three kinds -- a float64 host array, a float32 tensor, a transposed tensor (stride 1 along the
    detectors) -- on T coordinates whose azimuth sweeps once."""
    rng = np.random.default_rng(7)
    a = rng.standard_normal((D, T_fields))
    b = torch.as_tensor(rng.standard_normal((D, T_fields)).astype(np.float32))
    c = torch.as_tensor(rng.standard_normal((T_fields, D)).astype(np.float32)).t()
    assert c.stride(1) != 1
    coords = Coordinates(np.arange(T) / 10.0, np.linspace(0, 1, T), np.full(T, 1.0), offsets=np.zeros((D, 2)))
    dets = Detectors(np.zeros((D, 2)), [Band(center=150e9, width=30e9, name="f150")], np.zeros(D, int))
    return TOD({"a": a, "b": b, "c": c}, dets=dets, coords=coords, metadata={"site": "here"} if metadata is None else metadata, flags=flags)


def expected_sum(tod):
    a32, b32, c32 = (torch.as_tensor(v).to(torch.float32) for v in tod.data.values())
    return a32.clone().add_(b32).add_(c32)


def test_the_sum_and_the_copies():
    tod = make_tod(flags=torch.zeros((D, T), dtype=torch.uint8))
    before = {k: torch.as_tensor(v).clone() for k, v in tod.data.items()}
    data, signal, model, flags, into, ctx = tod._device_fields(None, None, CTX, "cpu")
    assert torch.equal(bits(signal), bits(expected_sum(tod)))
    assert list(data) == ["a", "b", "c"] and into == "a" and ctx is CTX and model is None
    assert flags.dtype == torch.uint8 and flags.is_contiguous()
    for k, x in data.items():
        src = torch.as_tensor(tod.data[k])
        assert x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() != src.data_ptr()
        assert torch.equal(x, src.to(torch.float32))
        x.add_(1.0)  # a copy: the TOD's own field does not move
        assert torch.equal(torch.as_tensor(tod.data[k]), before[k])
    _, _, model, _, into, _ = tod._device_fields(np.ones((D, T)), "c", CTX, "cpu")
    assert model.dtype == torch.float32 and model.is_contiguous() and into == "c"


def test_the_sum_alone():
    """Layer A returns the bits of the full upload and keeps no copy; a caller's device takes every field."""
    from maria_amd import tod as mtod

    tod = make_tod()
    want = bits(expected_sum(tod))
    s = tod._signal("cpu")
    assert torch.equal(bits(s), want) and s.dtype == torch.float32 and s.is_contiguous()
    assert torch.equal(bits(mtod.field_sum(tod.data.values(), torch.device("cpu"))), want)
    one = tod._signal("cpu", field="b")
    assert torch.equal(one, tod.data["b"]) and one.data_ptr() != tod.data["b"].data_ptr()
    assert mtod.field_device(tod.data.values(), "cpu") == torch.device("cpu")
    data, signal, dev = tod._field_copies("cpu")
    assert torch.equal(bits(signal), want) and dev == torch.device("cpu") and all(x.is_contiguous() for x in data.values())
    views, dev = tod._field_views("cpu")
    assert views["b"] is tod.data["b"] and views["c"].is_contiguous() and views["a"].dtype == torch.float32


def test_device_fields_refuses_in_order():
    """A bad ``into`` wins over fields that do not match the coordinates, and that over a model of the wrong shape."""
    long = make_tod(T_fields=T + 2)
    bad_model = np.zeros((D, T + 1))
    with pytest.raises(ValueError, match=re.escape("into 'zz': one of the fields ['a', 'b', 'c']")):
        long._device_fields(bad_model, "zz", CTX, "cpu")
    with pytest.raises(ValueError, match=re.escape(f"fields of shape ({D}, {T + 2}): the coordinates have {T} samples")):
        long._device_fields(bad_model, None, CTX, "cpu")
    with pytest.raises(ValueError, match=re.escape(f"model of shape ({D}, {T + 1}): the fields' ({D}, {T})")):
        make_tod()._device_fields(bad_model, None, CTX, "cpu")
    # stats and fit_beams refuse the same, in the same order, without the copies
    with pytest.raises(ValueError, match="the coordinates have"):
        long.stats(model=bad_model, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match="model of shape"):
        make_tod().stats(model=bad_model, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match="model of shape"):
        make_tod().fit_beams(frame="az/el", model=bad_model, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match=LAST):
        make_tod().stats(ctx=CTX, device="cpu")


def test_flag_glitches_checks_nothing_against_the_coordinates():
    """Its layer of the upload has no ``into``, no ``model`` and no check of T: fields of another length than the
    coordinates go as far as the first operator, which wants a device."""
    long = make_tod(T_fields=T + 2)
    with pytest.raises(ValueError, match=LAST):
        long.flag_glitches(ctx=CTX, device="cpu")


def test_the_copies_without_the_checks():
    long = make_tod(T_fields=T + 2)
    data, signal, dev = long._field_copies("cpu")
    assert tuple(signal.shape) == (D, T + 2) and torch.equal(bits(signal), bits(expected_sum(long)))


def test_a_derived_tod_carries_over():
    flags = torch.zeros((D, T), dtype=torch.uint8)
    tod = make_tod(flags=flags)
    calibrator = lambda data, to_krj: {k: v for k, v in data.items()}  # noqa: E731
    tod._calibrator = calibrator
    out = tod.with_offsets(np.ones((D, 2)))
    assert out.data is tod.data and out.flags is flags and out.metadata is tod.metadata and out.units is tod.units
    assert out._calibrator is calibrator and out.dets is not tod.dets and out.coords is not tod.coords
    assert np.array_equal(out.dets.offsets, np.ones((D, 2))) and np.array_equal(out.coords.offsets, np.ones((D, 2)))
    assert not tod.dets.offsets.any() and not tod.coords.offsets.any()
    krj = tod.to("K_RJ")
    assert krj.units == "K_RJ" and krj.dets is tod.dets and krj.coords is tod.coords and krj.metadata is tod.metadata
    assert krj.flags is flags and krj._calibrator is calibrator and krj.data is not tod.data and krj.to("K_RJ") is krj
    assert krj.to("pW").flags is krj.flags
    with pytest.raises(NotImplementedError):
        make_tod().to("K_RJ")  # no calibrator


def test_the_derived_tod_rule():
    flags = torch.zeros((D, T), dtype=torch.uint8)
    tod = make_tod(flags=flags)
    same = tod._derived()
    assert same is not tod and all(getattr(same, k) is getattr(tod, k) for k in ("data", "dets", "coords", "units", "metadata", "flags"))
    assert same._calibrator is None
    tod._calibrator = object()
    other = torch.ones((D, T), dtype=torch.uint8)
    out = tod._derived(data={"x": 1}, flags=other, units="K_RJ", record={"step": {"n": 1}})
    assert out.data == {"x": 1} and out.flags is other and out.units == "K_RJ" and out.dets is tod.dets and out.coords is tod.coords
    assert out._calibrator is tod._calibrator
    assert out.metadata is not tod.metadata and out.metadata == {"site": "here", "step": {"n": 1}} and tod.metadata == {"site": "here"}
    empty = tod._derived(record={})
    assert empty.metadata is not tod.metadata and empty.metadata == tod.metadata


BAD_GROUPS = 'groups must be a one-dimensional integer array with entries >= -1'


@pytest.mark.parametrize("method", ["remove_common_mode", "cut"])
def test_groups_refusals(method):
    tod = make_tod()
    call = lambda g: getattr(tod, method)(groups=g, ctx=CTX, device="cpu", **({"bounds": None} if method == "cut" else {}))  # noqa: E731
    with pytest.raises(ValueError, match=re.escape('groups \'array\': "band", None or an integer array')):
        call("array")
    for bad in ([[0, 0, 0]], [0.0, 0.0, 0.0], [0, 0, -2]):
        with pytest.raises(ValueError, match=re.escape(BAD_GROUPS)):
            call(bad)
    for good in ("band", None, [0, -1, 1]):  # as far as the first operator
        with pytest.raises(ValueError, match=LAST):
            call(good)


def test_cut_counts_the_groups_after_the_upload():
    with pytest.raises(ValueError, match=re.escape(f"groups must have one entry for each of the {D} detectors")):
        make_tod().cut(bounds=None, groups=[0, 0], ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match="the coordinates have"):  # the upload's refusal comes first
        make_tod(T_fields=T + 2).cut(bounds=None, groups=[0, 0], ctx=CTX, device="cpu")


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_groups_resolved(dtype):
    tod = make_tod()
    band = tod._groups("band", dtype)
    assert band.dtype == dtype and band.tolist() == [0, 0, 0] and tod._groups(None, dtype) is None
    given = tod._groups(np.array([0, -1, 1], np.int16), dtype)
    assert given.dtype == dtype and given.tolist() == [0, -1, 1]
    for bad in ("array", [[0, 0, 0]], [0.0, 0.0, 0.0], [0, 0, -2]):
        with pytest.raises(ValueError):
            tod._groups(bad, dtype)


def test_bounds_one_check_two_callers():
    tod = make_tod()
    message = re.escape("bounds must be a one-dimensional array of S + 1 >= 2 ascending integers")
    for bad in ([0, 9, 4, T], [0], [0.0, float(T)], [[0, T]]):
        with pytest.raises(ValueError, match=message):
            tod.filter_subscans(bounds=bad, ctx=CTX, device="cpu")
        with pytest.raises(ValueError, match=message):
            tod._segment_bounds(bad)
    with pytest.raises(ValueError, match=message):  # None or an array: no "subscans", no chunk length
        tod.filter_subscans(bounds="subscans", ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match=message):
        tod.filter_subscans(bounds=8, ctx=CTX, device="cpu")
    got = tod._segment_bounds([-3, 4, T + 9])
    assert got.dtype == np.int32 and got.tolist() == [0, 4, T]
    assert tod._segment_bounds(None).tolist() == [0, T] and tod._segment_bounds(16).tolist() == [0, 16, 32, T]
    assert tod._segment_bounds("subscans").tolist() == [0, T]
    with pytest.raises(ValueError, match=LAST):  # a good array goes as far as the first operator
        tod.filter_subscans(bounds=[-3, 4, T + 9], ctx=CTX, device="cpu")


def test_q_and_radius():
    from maria_amd.downsample import MAX_FACTOR, MIN_FACTOR
    from maria_amd.hwp import HWP

    tod = make_tod()
    for q in (MIN_FACTOR - 1, MAX_FACTOR + 1, 2.5):
        message = re.escape(f"q {q}: an integer in {MIN_FACTOR} .. {MAX_FACTOR}")
        with pytest.raises(ValueError, match=message):
            tod.downsample(q, ctx=CTX, device="cpu")
        with pytest.raises(ValueError, match=message):
            tod.demodulate(hwp=HWP(0.5), q=q, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match=LAST):
        tod.downsample(MIN_FACTOR, taps=np.ones(5) / 5, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match="no hwp given and no metadata"):
        tod.demodulate(q=2)
    with pytest.raises(ValueError, match="no hwp given and no metadata"):
        tod.remove_hwpss()
    # radius 0: the mask takes it (and goes on to want a device), the fit does not
    with pytest.raises(ValueError, match="the pointing must be on a device"):
        tod.mask_source(source=(0.0, 1.0), radius=0, frame="az/el", degrees=False, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match=re.escape("radius 0.0: finite and > 0")):
        tod.fit_beams(source=(0.0, 1.0), radius=0, frame="az/el", degrees=False, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match=re.escape("radius -1.0: finite and >= 0")):
        tod.mask_source(source=(0.0, 1.0), radius=-1, frame="az/el", degrees=False, ctx=CTX, device="cpu")
    with pytest.raises(ValueError, match="finite and > 0"):
        tod.fit_beams(radius=float("inf"), frame="az/el", ctx=CTX, device="cpu")


def test_the_sample_rate_where_there_is_none():
    """One sample: ``demodulate`` keeps its own message."""
    from maria_amd.hwp import HWP

    coords = Coordinates([0.0], [0.0], [1.0])
    tod = TOD({"a": np.zeros((D, 1), np.float32)}, dets=None, coords=coords)
    with pytest.raises(ValueError, match="demodulate needs at least two samples to know the sample rate"):
        tod.demodulate(hwp=HWP(0.5), q=2)


def test_one_spelling_of_t_and_of_the_sample_rate():
    tod = TOD({"a": np.zeros((D, 1), np.float32)}, dets=None, coords=Coordinates([0.0], [0.0], [1.0]))
    assert tod._T == 1 and make_tod()._T == T and make_tod()._sample_rate() == pytest.approx(10.0, rel=1e-12)


def test_tod_has_a_module_of_its_own():
    import maria_amd.sim
    import maria_amd.tod

    for name in ("TOD", "Coordinates", "sky_transform_stack"):
        assert getattr(maria_amd.sim, name) is getattr(maria_amd.tod, name)
    code = ("import sys; import maria_amd.tod; "
            "bad = [m for m in ('maria_amd.sim', 'maria_amd.atmosphere', 'torch') if m in sys.modules]; "
            "assert not bad, bad")
    root = os.path.dirname(os.path.dirname(os.path.abspath(maria_amd.tod.__file__)))
    done = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
