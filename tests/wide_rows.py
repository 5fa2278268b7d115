"""Rows of a [D, T] array laid out at a pitch past 2^31 elements (tests/test_gpu_wide_rows.py).

A pitch is only a stride: three rows of a few thousand samples at a pitch of 2^31 + 4 elements put row 1 past 2^31 and row
2 past 2^32 elements from the base pointer (for 4-byte elements past 2^33 and 2^34 bytes), so that an ``int`` or
``unsigned`` product of row and pitch, in elements or in bytes, lands somewhere else.  Only the rows and their guard strips
of the one big allocation (the arena) are ever touched.

The arithmetic is plain integers and needs no device: tests/test_host_wide_rows.py checks it.  Layout, in elements of the
array's own type, for row r of slot k (arrays that share one pitch argument are slots of one arena):

    start(r, k) = first + GUARD + k (T + 2 GUARD) + r pitch

  "aligned":  pitch = 2^31 + 4 (8-byte elements: 2^30 + 2), first = 0: every row as aligned as the arena itself
  "odd":      pitch = 2^31 + 5 (8-byte elements: 2^30 + 3), first = 1: row 0 is off the wide accesses' alignment and the rows' alignments differ

with GUARD = 64 sentinel elements (NaN, flags 255) in front of and behind every row.  The compact pitch T + 2 GUARD is the
one a call is handed in the wrong-pitch check: every access of it stays inside the arena's head, which is sentinel-filled
before any view is made."""

import numpy as np

D = 3
GUARD = 64
LAYOUTS = ("aligned", "odd")
PITCH_ELEMENTS = {"aligned": 2**31 + 4, "odd": 2**31 + 5}  # of 1- and 4-byte elements
MAX_SLOTS = 3  # arrays that share one pitch argument (mrx_tod_hwp_modulate: three inputs; mrx_tod_demodulate: three outputs)
ARENA_LIMIT = 18 * 2**30


def pitch(layout, itemsize):
    """The row pitch in elements: P for 1- and 4-byte elements; P / 2 for 8-byte ones, kept even or made odd."""
    P = PITCH_ELEMENTS[layout]
    if itemsize in (1, 4):
        return P
    assert itemsize == 8
    half = P // 2
    return half if layout == "aligned" else half | 1


def first(layout):
    """Elements between the arena's first byte and the first guard strip."""
    return 0 if layout == "aligned" else 1


def compact_pitch(T):
    return T + 2 * GUARD


def row_start(layout, itemsize, T, r, slot=0, ld=None):
    """Element index in the arena of sample 0 of row r of slot ``slot``; ``ld``: another pitch than the layout's."""
    return first(layout) + GUARD + slot * compact_pitch(T) + r * (pitch(layout, itemsize) if ld is None else ld)


def strips(layout, itemsize, T, slots=1):
    """[(start, stop)] of every guard strip, in elements: two a row."""
    out = []
    for k in range(slots):
        for r in range(D):
            s = row_start(layout, itemsize, T, r, k)
            out += [(s - GUARD, s), (s + T, s + T + GUARD)]
    return out


def head_elements(T, slots=1):
    """The sentinel-filled head: whatever a call at the compact pitch can reach, 3 (T + 128) + 64 for one slot."""
    return (slots + D - 1) * compact_pitch(T) + GUARD


def span_bytes(layout, itemsize, T, slots=1):
    """Bytes from the arena's start to the end of the last guard strip."""
    return itemsize * (row_start(layout, itemsize, T, D - 1, slots - 1) + T + GUARD)


def arena_bytes(T_max, slots=MAX_SLOTS):
    """One allocation that holds any array of at most T_max samples a row, of any element size, at either pitch:
    4 (2 P + T + guards) bytes and the little more that 8-byte rows and shared pitches take; a multiple of 16."""
    n = max(span_bytes(layout, size, T_max, slots) for layout in LAYOUTS for size in (1, 4, 8))
    n = max(n, 8 * head_elements(T_max, slots))
    return n + (-n) % 16


def sentinel(dtype):
    return float("nan") if np.dtype(dtype).kind == "f" else 255


class Arena:
    """The one big device allocation and the views into it.  ``torch.empty``: the arena is not filled."""

    def __init__(self, T_max, device="cuda:0"):
        import torch

        self.T_max = T_max
        self.bytes = arena_bytes(T_max)
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.placed = None

    def release(self):
        import torch

        self.buf = self.placed = None
        torch.cuda.empty_cache()

    def place(self, arrays, layout):
        """The [D, T] host arrays (one dtype, one T: the slots of one pitch argument) as wide views: head and guard strips
        sentinel-filled, rows copied in.  Returns (views, pitch)."""
        import torch

        a0 = np.asarray(arrays[0])
        T, size, slots = a0.shape[1], a0.dtype.itemsize, len(arrays)
        assert T <= self.T_max and slots <= MAX_SLOTS and span_bytes(layout, size, T, slots) <= self.bytes
        typed = self.buf.view(torch.as_tensor(np.array(a0[:0])).dtype)
        fill = sentinel(a0.dtype)
        typed[:head_elements(T, slots)].fill_(fill)
        for lo, hi in strips(layout, size, T, slots):
            typed[lo:hi].fill_(fill)
        P = pitch(layout, size)
        views = []
        for k, a in enumerate(arrays):
            a = np.asarray(a)
            assert a.shape == (D, T) and a.dtype == a0.dtype
            v = torch.as_strided(typed, (D, T), (P, 1), row_start(layout, size, T, 0, k))
            v.copy_(torch.as_tensor(np.array(a)))  # (a copy: the cases are read-only arrays)
            views.append(v)
        self.placed = (typed, layout, size, T, slots, fill)
        return views, P

    def guards_intact(self):
        """Do all guard strips of the last ``place`` still hold the sentinel?"""
        import torch

        typed, layout, size, T, slots, fill = self.placed
        got = torch.stack([typed[lo:hi] for lo, hi in strips(layout, size, T, slots)])
        return bool(torch.isnan(got).all()) if fill != fill else bool((got == fill).all())
