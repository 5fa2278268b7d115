"""The argument checks the TOD operators share (maria_amd._tod_args) on host tensors: the row check at its
edges, the output check in its two modes against every kind of view, and every public entry that takes ``out`` against
one table of legal, overlapping and in-place outputs."""

import numpy as np
import pytest
import torch

from maria_amd import _tod_args as A
from maria_amd import downsample, flagging, ground, hwp, jumps, regress, subscans, time_constants

D, T = 3, 40


def test_the_module_imports_no_operator():
    """It is the one home of the checks: nothing but ``__future__`` at module level (torch is imported inside the functions,
    so the module loads where torch does not), and of the package only ``_lib``."""
    import ast

    tree = ast.parse(open(A.__file__).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert [n.module for n in top] == ["__future__"]
    relative = {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level > 0}
    assert relative == {"_lib"}


def test_row_check_at_its_edges():
    flat = torch.zeros(64, dtype=torch.float32)
    assert A.check_x(torch.zeros((D, T))) == (D, T, T)
    assert A.check_x(torch.zeros((D, T + 8))[:, :T]) == (D, T, T + 8)
    # one row: stride(0) is never used, whatever it is, and the pitch is T
    assert A.check_x(flat.as_strided((1, 7), (3, 1))) == (1, 7, 7)
    assert A.check_x(flat.as_strided((1, 7), (0, 1))) == (1, 7, 7)
    # one sample a row: stride(1) is never used, the pitch is stride(0) and may be 1
    assert A.check_x(torch.zeros((4, 3))[:, :1]) == (4, 1, 3)
    assert A.check_x(flat.as_strided((4, 1), (2, 5))) == (4, 1, 2)
    assert A.check_x(flat.as_strided((4, 1), (1, 1))) == (4, 1, 1)
    assert A.check_x(flat.as_strided((1, 1), (9, 9))) == (1, 1, 1)
    for bad, msg in ((flat.as_strided((3, 8), (4, 1)), "row pitch >= T"),    # rows that run into each other
                     (flat.as_strided((3, 8), (0, 1)), "row pitch >= T"),    # an expanded row
                     (torch.zeros((D, 2 * T))[:, ::2], "unit stride"),
                     (torch.zeros((T, D)).t(), "unit stride"),
                     (torch.zeros((D, T), dtype=torch.float64), "float32"),
                     (torch.zeros(T), r"\[D, T\]"), (torch.zeros((1, D, T)), r"\[D, T\]"), (np.zeros((D, T), np.float32), r"\[D, T\]"),
                     (torch.zeros((0, T)), "D >= 1"), (torch.zeros((D, 0)), "T >= 1")):
        with pytest.raises(ValueError, match=msg):
            A.check_x(bad)
    with pytest.raises(ValueError, match="^s_i must be"):
        A.check_x(torch.zeros(T), "s_i")


def test_same_shape_check_takes_the_dtype():
    x = torch.zeros((D, T))
    assert A.check_like(torch.zeros((D, T + 4))[:, :T], "model", x, D, T) == T + 4
    assert A.check_like(torch.zeros((D, T), dtype=torch.uint8), "flags", x, D, T, "uint8") == T
    assert A.check_like(torch.zeros((1, T)).as_strided((1, T), (5, 1)), "model", x[:1], 1, T) == T
    with pytest.raises(ValueError, match=rf"^flags must be a \[{D}, {T}\] uint8 tensor on x's device$"):
        A.check_like(x, "flags", x, D, T, "uint8")
    with pytest.raises(ValueError, match=rf"^model must be a \[{D}, {T}\] float32 tensor on x's device$"):
        A.check_like(torch.zeros((D, T), dtype=torch.uint8), "model", x, D, T)
    with pytest.raises(ValueError, match="^out must have unit stride along time and a row pitch >= T_out$"):
        A.check_like(torch.zeros((D, 2 * T))[:, ::2], "out", x, D, T, length="T_out")


def _views():
    """x and the outputs of the table below, all views of fresh buffers."""
    padded = torch.zeros((D, T + 8))
    rows = torch.zeros((D + 1, T))
    halves = torch.zeros((2 * D, T))
    x = padded[:, :T]
    return {
        "x itself": (x, x),
        "an equal view": (x, x[:, :]),
        "a view one sample on": (x, padded[:, 1:T + 1]),
        "a view one row on": (rows[:-1], rows[1:]),
        "the other half of the buffer": (halves[:D], halves[D:]),
        "a tensor of its own": (x, torch.zeros((D, T))),
        "its own pitch": (x, torch.zeros((D, T + 3))[:, :T]),
    }


@pytest.mark.parametrize("in_place", [False, True])
def test_output_check_in_both_modes(in_place):
    accepted = {"the other half of the buffer", "a tensor of its own", "its own pitch"} | ({"x itself", "an equal view"} if in_place else set())
    message = "^out must be x or must not overlap it$" if in_place else "^out must not overlap x$"
    for name, (x, out) in _views().items():
        if name in accepted:
            A.check_out(out, x, D, T, in_place=in_place)
        else:
            with pytest.raises(ValueError, match=message):
                A.check_out(out, x, D, T, in_place=in_place)
                pytest.fail(name)
    # the two halves touch: the first ends where the second begins
    x, out = _views()["the other half of the buffer"]
    assert A.byte_span(x)[1] == A.byte_span(out)[0] and not A.overlaps(x, out)
    x = torch.zeros((D, T))
    for bad, msg in ((torch.zeros((D, T), dtype=torch.float64), "float32 tensor on x's device"),
                     (torch.zeros((D, T), dtype=torch.uint8), "float32 tensor on x's device"),
                     (torch.zeros((D, T + 1)), "float32 tensor on x's device"), (torch.zeros((D + 1, T)), "float32 tensor on x's device"),
                     (torch.zeros(D * T), "float32 tensor on x's device"), (np.zeros((D, T), np.float32), "float32 tensor on x's device"),
                     (torch.zeros((D, T), device="meta"), "float32 tensor on x's device"),
                     (torch.zeros((D, 2 * T))[:, ::2], "unit stride"), (torch.zeros((1, T)).expand(D, T), "row pitch >= T")):
        with pytest.raises(ValueError, match=msg):
            A.check_out(bad, x, D, T, in_place=in_place)
    # a shorter output (decimate): its own length in shape and message, and strict against the rows it is made from
    x = torch.zeros((D, T + 8))[:, :T]
    A.check_out(torch.zeros((D, T // 2)), x, D, T // 2, length="T_out")
    with pytest.raises(ValueError, match="overlap"):
        A.check_out(x[:, :T // 2], x, D, T // 2, length="T_out")
    with pytest.raises(ValueError, match="row pitch >= T_out"):
        A.check_out(torch.zeros((1, T // 2)).expand(D, T // 2), x, D, T // 2, length="T_out")


def test_small_checks():
    assert A.check_count(8.0, "K", 8) == 8 and A.check_min_hits(0) == 0 and A.check_min_hits(True) == 1
    assert A.check_sign(-1) == -1 and A.check_sign(1.0) == 1 and A.check_scratch_bytes(1) == 1
    for fn, bad in ((lambda v: A.check_count(v, "K", 8), (0, 9, 1.5)), (A.check_min_hits, (-1, 1.5)), (A.check_sign, (0, 2, -1.5)),
                    (A.check_scratch_bytes, (0, -4, 1.5)), (lambda v: A.check_min_hits(v, allow_bool=False), (True, -1))):
        for v in bad:
            with pytest.raises(ValueError):
                fn(v)
    a = np.arange(3)
    assert A.to_numpy(a) is a and A.to_numpy([1, 2]) == [1, 2]
    assert np.array_equal(A.to_numpy(torch.arange(3.0, requires_grad=True)), [0.0, 1.0, 2.0])


# every public entry that takes ``out``: (name, strict, call(x, out)); x is [D, T] float32 on the host, so that a call that
# passes every check is refused last, for not being on a device
def _entries():
    K = 2
    bins = np.arange(T) % 4
    template = torch.zeros((D, 4))
    B, a = torch.zeros((1, K, T)), torch.zeros((D, K), dtype=torch.float64)
    bounds, seg = np.array([0, T]), torch.zeros((D, 1, K), dtype=torch.float64)
    pole = np.array([0.0, 0.5, 0.9])
    no_jumps = (np.zeros(D + 1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    carrier = np.zeros((T, 2))

    def modulate(x, out):
        s_c, s_s = (torch.zeros((D, x.stride(0)))[:, :T] for _ in range(2))  # one row pitch with s_i
        return hwp.modulate(x, s_c, s_s, carrier, out=out)

    return [
        ("median_residual", True, lambda x, out: flagging.median_residual(x, out=out)),
        ("step_statistic", True, lambda x, out: jumps.step_statistic(x, 8, out=out)),
        ("decimate", True, lambda x, out: downsample.decimate(x, 2, taps=np.ones(3), out=out)),
        ("fix_jumps", False, lambda x, out: jumps.fix_jumps(x, *no_jumps, out=out)),
        ("apply_template", False, lambda x, out: ground.apply_template(x, bins, template, out=out)),
        ("regress.apply", False, lambda x, out: regress.apply(x, B, a, out=out)),
        ("subscans.apply", False, lambda x, out: subscans.apply(x, bounds, seg, out=out)),
        ("time_constants.apply", False, lambda x, out: time_constants.apply(x, pole, out=out)),
        ("time_constants.deconvolve", False, lambda x, out: time_constants.deconvolve(x, pole, out=out)),
        ("modulate", False, modulate),
    ]


@pytest.mark.parametrize("name, strict, call", _entries(), ids=[e[0] for e in _entries()])
def test_every_entry_with_out_follows_the_one_rule(name, strict, call):
    """A legal ``out`` passes every check (the call is refused as a host tensor, the last refusal); a view one sample on
    in the same buffer is refused as an overlap; ``out = x`` and an equal view of it are an overlap for the strict entries
    and legal for the others.  decimate's output is shorter than x, so its "x" is the view of x's rows of that length."""
    T_out = T // 2 if name == "decimate" else T
    padded = torch.zeros((D, T + 8))
    x = padded[:, :T]
    for legal in (None, torch.zeros((D, T_out)), torch.zeros((D, T_out + 5))[:, :T_out]):
        with pytest.raises(ValueError, match="must be a device tensor$"):
            call(x, legal)
    with pytest.raises(ValueError, match="overlap"):
        call(x, padded[:, 1:T_out + 1])
    for same in ((x if T_out == T else x[:, :T_out]), x[:, :T_out]):
        with pytest.raises(ValueError, match="overlap" if strict else "must be a device tensor$"):
            call(x, same)
    for bad in (torch.zeros((D, T_out), dtype=torch.float64), torch.zeros((D, T_out + 1)), torch.zeros((D, T_out), device="meta")):
        with pytest.raises(ValueError, match="float32 tensor on"):
            call(x, bad)
