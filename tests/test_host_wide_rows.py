"""The wide-row layout's arithmetic (tests/wide_rows.py) and the completeness of tests/test_gpu_wide_rows.py's table
against include/mrx.h.  No device."""

import os
import re

import pytest
import test_gpu_wide_rows as gw
import wide_rows as wr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrx.h")
LENGTHS = [1, 515, gw.T0, gw.T_MAX]


def pitched_entries():
    """entry -> the names of its ``size_t ld*`` parameters, from the declarations of the header."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(mrx_\w+)\s*\(([^;{}]*)\)\s*;", text):
        lds = re.findall(r"\bsize_t\s+(ld\w*)", args)
        if lds:
            out[name] = sorted(lds)
    return out


@pytest.mark.parametrize("itemsize", [1, 4, 8])
@pytest.mark.parametrize("layout", wr.LAYOUTS)
def test_the_rows_cross_the_thresholds(layout, itemsize):
    """Rows 1 and 2 start past 2^31 and 2^32 elements (8-byte rows: 2^30 and 2^31), so for 4- and 8-byte elements past 2^33
    and 2^34 bytes: past what a signed and an unsigned 32-bit offset hold, in elements and in bytes."""
    lo = 2**31 if itemsize < 8 else 2**30
    for T in LENGTHS:
        for slot in range(wr.MAX_SLOTS):
            r0, r1, r2 = (wr.row_start(layout, itemsize, T, r, slot) for r in range(3))
            assert r0 + T < 2**24 and lo < r1 < 2 * lo < r2 < 3 * lo
            assert r1 - r0 == r2 - r1 == wr.pitch(layout, itemsize) >= T
            if itemsize >= 4:
                assert itemsize * r1 > 2**33 and itemsize * r2 > 2**34
            assert itemsize * r1 > 2**31 and itemsize * r2 > 2**32


@pytest.mark.parametrize("itemsize", [1, 4, 8])
@pytest.mark.parametrize("layout", wr.LAYOUTS)
def test_strips_and_rows_do_not_overlap_and_fit_the_arena(layout, itemsize):
    for T in LENGTHS:
        for slots in range(1, wr.MAX_SLOTS + 1):
            strips = wr.strips(layout, itemsize, T, slots)
            assert len(strips) == 2 * wr.D * slots and all(hi - lo == wr.GUARD for lo, hi in strips)
            rows = [(wr.row_start(layout, itemsize, T, r, k), wr.row_start(layout, itemsize, T, r, k) + T) for k in range(slots) for r in range(wr.D)]
            spans = sorted(strips + rows)
            assert spans[0][0] >= 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
            assert all(any(lo == hi_r for lo, _ in strips) and any(hi == lo_r for _, hi in strips) for lo_r, hi_r in rows)  # a strip either side
            assert itemsize * spans[-1][1] == wr.span_bytes(layout, itemsize, T, slots) <= wr.arena_bytes(gw.T_MAX)
            # the head holds every row of slot and row 0, and whatever a call at the compact pitch reaches
            head = wr.head_elements(T, slots)
            reach = max(wr.row_start(layout, itemsize, T, r, k, ld=wr.compact_pitch(T)) + T for k in range(slots) for r in range(wr.D))
            assert reach <= head and itemsize * head <= wr.arena_bytes(gw.T_MAX)
            assert head == 3 * (T + 128) + 64 or slots > 1


@pytest.mark.parametrize("itemsize", [1, 4, 8])
def test_alignment_is_kept_or_broken_as_claimed(itemsize):
    """ "aligned": every row starts on a multiple of 16 bytes (flags: of 4) from the arena's first byte; "odd": the pitch is
    odd, row 0 starts off that multiple and the three rows' alignments all differ (8-byte rows, two to 16 bytes: alternate)."""
    wide = 16 // itemsize if itemsize > 1 else 4
    for T in LENGTHS:
        for slot in range(wr.MAX_SLOTS):
            if T % wide == 0 or slot == 0:
                starts = [wr.row_start("aligned", itemsize, T, r, slot) for r in range(3)]
                assert all(s % wide == 0 for s in starts), (T, slot, starts)
            starts = [wr.row_start("odd", itemsize, T, r, slot) for r in range(3)]
            assert wr.pitch("odd", itemsize) % 2 == 1 and len({s % wide for s in starts}) == min(3, wide)
            assert slot or starts[0] % wide == 1
    assert wr.pitch("aligned", itemsize) % wide == 0 and wr.pitch("aligned", 8) % 2 == 0
    assert wr.pitch("aligned", 4) == 2**31 + 4 and wr.pitch("odd", 4) == 2**31 + 5 and wr.first("odd") == 1 and wr.first("aligned") == 0
    assert wr.pitch("aligned", 8) == 2**30 + 2 and wr.pitch("odd", 8) == 2**30 + 3


def test_the_arena_is_one_allocation_of_at_most_18_gib():
    n = wr.arena_bytes(gw.T_MAX)
    assert 2**34 < n <= wr.ARENA_LIMIT == 18 * 2**30 and n % 16 == 0
    assert n - 2**34 < 2**20  # 4 (2 P + T + guards) bytes and the little more of the module's docstring: 17.2 GB


def test_every_pitched_entry_is_in_the_table_or_excluded():
    """Each entry of the header with a ``size_t ld*`` parameter is in the GPU module's table with exactly its pitch
    arguments as roles, or in its exclusion list with a reason; nothing else is in either.  A new pitched entry fails
    here until it is covered."""
    header = pitched_entries()
    assert len(header) == 59
    table, excluded = set(gw.TABLE), set(gw.EXCLUDED)
    assert not table & excluded
    assert table | excluded == set(header), (sorted(set(header) - table - excluded), sorted((table | excluded) - set(header)))
    assert len(table) == 42 and len(excluded) == 17 and all(isinstance(r, str) and len(r) > 20 for r in gw.EXCLUDED.values())
    for entry in table:
        assert gw.table_roles(entry) == header[entry], (entry, gw.table_roles(entry), header[entry])
        builders, roles = gw.TABLE[entry]
        assert builders and len(set(roles)) == len(roles)
        assert all(token in [r for r in roles if "+" not in r] for r in roles for token in r.split("+")), entry  # in place: also alone
    assert len(gw.PARAMS) == sum(len(roles) for _, roles in gw.TABLE.values()) and len(set(gw.IDS)) == len(gw.IDS)


def test_the_completeness_check_notices_a_missing_entry(monkeypatch):
    table = dict(gw.TABLE)
    del table["mrx_tod_gram"]
    monkeypatch.setattr(gw, "TABLE", table)
    with pytest.raises(AssertionError):
        test_every_pitched_entry_is_in_the_table_or_excluded()
    roles = dict(gw.TABLE, mrx_tod_gram=(gw.only(gw.gram), ("ld_x", "ld_m")))
    monkeypatch.setattr(gw, "TABLE", roles)
    with pytest.raises(AssertionError):
        test_every_pitched_entry_is_in_the_table_or_excluded()
