"""Every coarse sample of the atmosphere samplers against an exact line of sight: atm_sample_px_kernel in its
plain, two-step, resident (kPipe) and global-table instances, atm_sample_kernel's literal, chain and array-search routes, and
the sampler role of the one-launch synthesis -- on screens that turn a position error into a value error at full size.  Per
layer and axis an index ramp and a triangle wave with that one layer lit (the downloaded float64 pwv is then the position
itself); the whole stack on white noise; the rim of a cropped grid sample by sample; and the band lookup of every run
against a float64 evaluation at the device's own pwv.  Every sample is judged; eps and the bounds come from
tests/atm_los_ref.py alone (tests/test_host_atm_los_ref.py checks them on the CPU).

Every test prints one line of figures ("atm los: ..."), the ones DESIGN 3.41 quotes."""

import ctypes as C
from dataclasses import dataclass, field

import atm_los_ref as ar
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAIN, LITERAL, TIMES, CHUNK, WGS = 0, 1, 2, 3, 6  # MRX_OPT_POINTING_CHAIN, _AXIS_LITERAL, _SAMPLE_TIMES, _SAMPLE_CHUNK, _SAMPLE_WGS_PER_CU


@dataclass(frozen=True)
class Route:
    opts: dict = field(default_factory=dict)
    eps: str = "pixel"      # which eps of atm_los_ref.Case.eps the route is held to
    tables: tuple = None    # band tables of this many (pwv, el) nodes instead of the case's
    synth: dict = None      # DevicePath.synthesize with these arguments instead of DevicePath.sample


ROUTES = {
    "pixel": Route(),
    "times2": Route({TIMES: 2, CHUNK: 6}),            # odd Ta: the last pair straddles the end
    "pipe": Route({WGS: 3, TIMES: 1, CHUNK: 64}),      # kPipe; 64 steps x 7 layers: two trips of the anchor loop
    "pipe-times2": Route({WGS: 3, TIMES: 2, CHUNK: 6}),
    "global-tables": Route(tables=(80, 90)),          # kLdsTables = false
    "literal": Route({LITERAL: 1, TIMES: 1}, eps="literal"),
    "literal-times2": Route({LITERAL: 1, TIMES: 2}, eps="literal"),
    "literal-times4": Route({LITERAL: 1, TIMES: 4}, eps="literal"),
    "chain": Route({CHAIN: 1}, eps="literal"),
    "general": Route(eps="general"),                  # atm_sample_kernel's default rule: pixels beside array searches
    "general-times2": Route({TIMES: 2}, eps="general"),
    "general-times4": Route({TIMES: 4, CHUNK: 8}, eps="general"),
    "synth-2x32": Route(synth=dict(block_rows=256, sampler_wgs_per_cu=2, chunk=32)),
    "synth-0x8": Route(synth=dict(block_rows=256, sampler_wgs_per_cu=0, chunk=8)),
}
S_ROUTES = ["pixel", "times2", "pipe", "pipe-times2", "global-tables", "literal", "literal-times2", "literal-times4", "chain",
            "synth-2x32", "synth-0x8"]
OTHER = [("W", "pixel"), ("W", "times2"), ("W", "pipe-times2"), ("W", "synth-2x32"),
         ("F", "pixel"), ("F", "pipe"), ("F", "literal"), ("F", "synth-0x8"),
         ("R", "pixel"), ("R", "times2"), ("R", "pipe"), ("R", "synth-2x32"),
         ("N", "general"), ("N", "general-times2"), ("N", "general-times4"),
         ("L", "pixel"), ("L", "pipe-times2"), ("L", "synth-0x8")]


class Bench:
    """One case on the device through one route: binds screens, runs, downloads; atm_los_ref.Judge judges every sample."""

    def __init__(self, ctx, case, route):
        from maria_amd.pipeline import DevicePath

        self.ctx, self.case, self.route = ctx, case, route
        base = case.problem if route.tables is None else case.with_tables(*route.tables)
        self.problem = dict(base, layers=[dict(l) for l in base["layers"]])
        self.n_layers = len(self.problem["layers"])
        self.judge = ar.Judge(case, route.eps)
        self._bind([np.zeros(s, np.float32) for s in case.shapes], [0.0] * self.n_layers)
        self.path = DevicePath(self.problem, device="cuda:0", ctx=ctx, keep_pwv=True)

    def _bind(self, screens, rms):
        for layer, v, r in zip(self.problem["layers"], screens, rms):
            layer["values"], layer["pwv_rms"] = v, float(r)

    def run(self, screens, rms):
        """The pwv [D, Ta] float64 of one run with these screens and layer amplitudes; the flags and the band lookup of the
        run are judged here."""
        import torch

        from maria_amd import _lib
        from maria_amd._lib import ptr

        path, ctx = self.path, self.ctx
        self._bind(screens, rms)
        path.set_screens(screens)
        path.clear_flags()
        path.d_pwv.fill_(-7.0)
        saved = {k: ctx.get_option(k) for k in self.route.opts}
        try:
            for k, v in self.route.opts.items():
                ctx.set_option(k, v)
            if self.route.synth is None:
                path.sample()
            else:
                path.synthesize(**self.route.synth)
        finally:
            for k, v in saved.items():
                ctx.set_option(k, v)
        pwv, loading = path.coarse_pwv().cpu().numpy(), path.coarse_loading().cpu().numpy()
        torch.cuda.synchronize()
        word = C.c_uint32()
        ctx.call("mrx_read_flags", ptr(path.d_flags), C.byref(word))
        path.clear_flags()
        assert not word.value & _lib.FLAG_TABLE_OOB
        assert bool(word.value & _lib.FLAG_SCREEN_OOB) == bool(np.isnan(pwv).any())
        if not self.judge.must_nan.any():
            assert word.value == 0
        self.judge.band(self.problem, pwv, loading)
        return pwv

    def axis(self, l, axis, kind):
        self.judge.axis(l, axis, kind, self.run(*self.judge.axis_run(l, axis, kind)))

    def stack(self):
        self.judge.stack(self.run(self.case.noise, self.judge.profile))

    def report(self, name):
        w, eps = self.judge.worst, self.judge.eps
        print(f"atm los: case {self.case.name} route {name}: largest |device - exact| = {w['position']:.2e} pixel "
              f"(eps up to {eps.max():.2e}), white-noise stack |err| / bound <= {w['stack']:.3f}, band lookup <= {w['band']:.3f}")


def _bench(gpu_ctx, case_name, route_name):
    case, route = ar.case(case_name), ROUTES[route_name]
    bench = Bench(gpu_ctx, case, route)
    uniform_axes, tables_in_lds = bench.path.plan_info()
    assert tables_in_lds == (route.tables is None)
    # (case F too: 31 km from the origin the axes still verify, and the plan takes the pixel path)
    assert uniform_axes == (4 if case_name == "N" else 2 * bench.n_layers)
    return bench


@pytest.mark.parametrize("route", S_ROUTES)
def test_every_route_on_ramps_waves_and_noise(gpu_ctx, route):
    """Case S (7 layers: every slot of the kPxStages = 3 ring and its tail) through every route, with all three kinds of
    screen: per layer and axis the index ramp and the triangle wave, then the white-noise stack."""
    bench = _bench(gpu_ctx, "S", route)
    for l in range(bench.n_layers):
        for axis in (0, 1):
            bench.axis(l, axis, "ramp")
            bench.axis(l, axis, "tri")
    bench.stack()
    bench.report(route)


@pytest.mark.parametrize("case,route", OTHER, ids=[f"{c}-{r}" for c, r in OTHER])
def test_wide_far_cropped_and_nonuniform_grids(gpu_ctx, case, route):
    """W (|delta| past 40 pixels), F (axes 31 km from the origin: the float64 anchor keeps the pixel route inside S's eps,
    the literal route is held to its own), R (samples off each of the four sides: NaN exactly beyond the rim) and N (the
    general kernel's array search beside its pixel path) and L (6000 pixels from the grid's first node: the anchor must be made
    in float64): the white-noise stack and the triangle waves of the top and the
    bottom layer."""
    bench = _bench(gpu_ctx, case, route)
    for l in (0, bench.n_layers - 1):
        for axis in (0, 1):
            bench.axis(l, axis, "tri")
    bench.stack()
    if case == "R":
        assert bench.judge.must_nan.any() and np.isnan(bench.path.coarse_pwv().cpu().numpy()).any()
    bench.report(route)
