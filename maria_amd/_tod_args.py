"""The argument checks shared by the operators on a [D, T] TOD (flagging, downsample, ground, regress, jumps, subscans,
time_constants, cuts, hwp, beamfit, covariance, sky_polynomial, lines).  Every check raises ValueError and touches no device, so the operators
refuse on host tensors what they refuse on device tensors.  torch and ``_lib`` are imported inside the functions, and no
operator module is imported at all: this module loads where no device and no library is."""

from __future__ import annotations


def row_pitch(t):
    """The samples between two rows of a [D, T] tensor; T where there is one row only."""
    return t.stride(0) if t.shape[0] > 1 else int(t.shape[1])


def check_x(x, name="x"):
    """(D, T, row pitch) of a [D, T] float32 tensor with unit stride along time."""
    import torch

    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{name} must be a [D, T] float32 tensor")
    D, T = int(x.shape[0]), int(x.shape[1])
    if D < 1 or T < 1:
        raise ValueError(f"{name} of shape {tuple(x.shape)}: need D >= 1 rows of T >= 1 samples")
    if (T > 1 and x.stride(1) != 1) or (D > 1 and x.stride(0) < T):
        raise ValueError(f"{name} must have unit stride along time and a row pitch >= T")
    return D, T, row_pitch(x)


def check_like(a, name, x, D, T, dtype="float32", length="T"):
    """The row pitch of ``a``, a [D, T] tensor of ``dtype`` (torch's name of it) on x's device with unit stride along
    time.  ``length``: what the message calls T."""
    import torch

    if not isinstance(a, torch.Tensor) or a.dtype != getattr(torch, dtype) or tuple(a.shape) != (D, T) or a.device != x.device:
        raise ValueError(f"{name} must be a [{D}, {T}] {dtype} tensor on x's device")
    if (T > 1 and a.stride(1) != 1) or (D > 1 and a.stride(0) < T):
        raise ValueError(f"{name} must have unit stride along time and a row pitch >= {length}")
    return row_pitch(a)


def byte_span(t):
    """[first, past-the-last) byte addresses a 2-D tensor's elements lie in."""
    last = sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def overlaps(a, b):
    """Do the byte spans of two tensors meet?  (Rows interleaved in one buffer count as meeting.)"""
    (a0, a1), (b0, b1) = byte_span(a), byte_span(b)
    return a0 < b1 and b0 < a1


def same_rows(a, b):
    """Are two checked [D, T] tensors of one dtype the same memory: the same first byte and the same row pitch?"""
    return a is b or (a.data_ptr() == b.data_ptr() and row_pitch(a) == row_pitch(b))


def check_out(out, x, D, T, in_place=False, length="T"):
    """A caller's ``out`` for a [D, T] float32 result of ``x``: the refusals of ``check_like``, then the overlap rule.
    Strict (the kernel reads neighbouring samples): ``out`` must not overlap ``x`` at all.  ``in_place``: ``out`` may be
    ``x`` or an equal view of it (``same_rows``); every other overlap is refused.  Not for ``out`` None: the caller
    allocates, before or after its "must be a device tensor" refusal as it did."""
    check_like(out, "out", x, D, T, length=length)
    if overlaps(out, x) and not (in_place and same_rows(out, x)):
        raise ValueError("out must be x or must not overlap it" if in_place else "out must not overlap x")


def check_count(n, name, hi):
    if int(n) != n or not 1 <= int(n) <= hi:
        raise ValueError(f"{name} {n}: an integer in 1 .. {hi}")
    return int(n)


def check_min_hits(min_hits, allow_bool=True):
    if (not allow_bool and isinstance(min_hits, bool)) or int(min_hits) != min_hits or int(min_hits) < 0:
        raise ValueError(f"min_hits {min_hits}: an integer >= 0")
    return int(min_hits)


def check_sign(sign):
    if sign not in (-1, 1):
        raise ValueError(f"sign {sign}: -1 or +1")
    return int(sign)


def check_scratch_bytes(scratch_bytes):
    if int(scratch_bytes) != scratch_bytes or scratch_bytes < 1:
        raise ValueError(f"scratch_bytes {scratch_bytes}: a positive integer")
    return int(scratch_bytes)


def to_numpy(a):
    """A tensor's values as a host array; anything else as it is."""
    import torch

    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def context(ctx, x):
    """``ctx``, or a Context on x's device bound to torch's current stream there, made for the call."""
    import torch

    from ._lib import Context

    if ctx is None:
        ctx = Context(x.device.index or 0)
        ctx.set_stream(torch.cuda.current_stream(x.device))
    return ctx
