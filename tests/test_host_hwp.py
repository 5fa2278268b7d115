"""maria_amd.hwp on the host: the filter design, the conventions, the demodulated detector table, the
premise of the mappers' change, the reference formula's own recovery of Q and U, and the refusals, which come before any
device call."""

import hwp_ref as ref
import numpy as np
import pytest

from maria_amd import hwp
from maria_amd.instrument import Band, Detectors
from maria_amd.map import mueller_row


def test_design_taps_meet_their_claim():
    """An odd count, unit DC gain, and the stop band from stop_edge f_hwp to Nyquist below -atten_db + 3 dB (the
    allowance is for Kaiser's empirical formula), on an FFT of the taps at 16x zero padding."""
    for fs, f, atten in ((200.0, 2.0, 120.0), (400.0, 8.0, 120.0), (128.0, 2.0, 120.0), (100.0, 2.5, 80.0)):
        h = hwp.design_taps(fs, f, atten_db=atten)
        assert h.dtype == np.float64 and h.size % 2 == 1 and h.size <= 1025
        assert abs(h.sum() - 1.0) <= 1e-12
        n = 16 * h.size
        gain = np.abs(np.fft.rfft(h, n)) / abs(h.sum())
        freq = np.fft.rfftfreq(n, 1.0 / fs)
        worst = 20 * np.log10(gain[freq >= 2.0 * f].max())
        print(f"fs {fs} f_hwp {f}: {h.size} taps, stop band {worst:.1f} dB")
        assert worst <= -atten + 3.0
        assert 20 * np.log10(gain[freq <= 0.5 * f].min()) >= -0.01  # and the pass band is flat
    with pytest.raises(ValueError, match="1025"):
        hwp.design_taps(1000.0, 2.0)
    with pytest.raises(ValueError):
        hwp.design_taps(10.0, 8.0)  # the stop edge beyond Nyquist


def test_max_factor():
    assert hwp.max_factor(400.0, 8.0, 0.5, 2.0) == 20
    assert hwp.max_factor(200.0, 2.0, 0.5, 2.0) == 40
    assert hwp.max_factor(100.0, 2.5) == 16
    for fs, f in ((400.0, 8.0), (200.0, 2.0), (173.0, 3.1)):
        q = hwp.max_factor(fs, f, 0.5, 2.0)
        assert fs / q - 2.0 * f >= 0.5 * f * (1 - 1e-9) and fs / (q + 1) - 2.0 * f < 0.5 * f


def test_angle_and_carrier():
    t = 1.7e9 + np.arange(1000) / 200.0
    h = hwp.HWP(frequency=2.0, phase=0.3, direction=-1)
    chi = h.angle(t)
    assert chi.dtype == np.float64 and chi[0] == 0.3
    np.testing.assert_array_equal(chi, 0.3 - 2 * np.pi * 2.0 * (t - t[0]))
    c = hwp.carrier(chi)
    assert c.shape == (1000, 2) and c.dtype == np.float64 and c.flags.c_contiguous
    np.testing.assert_array_equal(c[:, 0], np.cos(4 * chi))
    np.testing.assert_array_equal(c[:, 1], np.sin(4 * chi))
    assert hwp.HWP.from_metadata(h.to_metadata()).to_metadata() == {"frequency": 2.0, "phase": 0.3, "direction": -1}
    for bad in (dict(frequency=0.0), dict(frequency=np.nan), dict(frequency=1.0, direction=2), dict(frequency=1.0, phase=np.inf)):
        with pytest.raises(ValueError):
            hwp.HWP(**bad)


def _dets():
    bands = [Band(center=90e9, width=30e9, name="f090"), Band(center=150e9, width=30e9, name="f150")]
    gamma = np.array([0.0, np.nan, 0.7, np.pi / 2, np.nan])
    return Detectors(np.arange(10.0).reshape(5, 2) * 1e-3, bands, [0, 1, 1, 0, 0], primary_size=[6, 7, 8, 9, 10], gamma=gamma,
                     time_constant=[0, 1e-3, 2e-3, 0, 0])


def test_stokes_rows_without_an_override_are_the_mueller_rows():
    d = _dets()
    assert d.stokes is None
    np.testing.assert_array_equal(d.stokes_rows(), mueller_row(d.gamma))
    # the premise of the mappers' unit_i_response: a row's I weight IS mueller00, bit for bit
    g = np.concatenate([d.gamma, np.random.default_rng(0).uniform(-4, 4, 100)])
    many = Detectors(np.zeros((g.size, 2)), d.bands, np.zeros(g.size, int), gamma=g)
    np.testing.assert_array_equal(many.mueller00()[:, None], mueller_row(g)[:, :1])
    with pytest.raises(ValueError):
        Detectors(np.zeros((3, 2)), d.bands, np.zeros(3, int), stokes=np.zeros((3, 3)))


def test_demodulated_detectors():
    d = _dets()
    m = hwp.demodulated_detectors(d)
    pol = np.array([0, 2, 3])
    np.testing.assert_array_equal(hwp.polarized_rows(d), pol)
    idx = np.concatenate([np.arange(5), pol, pol])
    assert m.n == 11
    np.testing.assert_array_equal(m.offsets, d.offsets[idx])
    np.testing.assert_array_equal(m.band_index, d.band_index[idx])
    np.testing.assert_array_equal(m.primary_size, d.primary_size[idx])
    np.testing.assert_array_equal(m.time_constant, d.time_constant[idx])
    np.testing.assert_array_equal(m.gamma, np.concatenate([d.gamma, -d.gamma[pol], np.pi / 4 - d.gamma[pol]]))
    rows = m.stokes_rows()
    assert rows.shape == (11, 4)
    np.testing.assert_array_equal(rows[:5], np.stack([d.mueller00(), np.zeros(5), np.zeros(5), np.zeros(5)], axis=1))
    for block, g in ((rows[5:8], -d.gamma[pol]), (rows[8:], np.pi / 4 - d.gamma[pol])):
        w = mueller_row(g)
        np.testing.assert_array_equal(block, np.stack([np.zeros(3), w[:, 1], w[:, 2], np.zeros(3)], axis=1))
    # the Q row of angle 0 sees +Q, its U row +U; at pi / 2 both change sign (d = w_I [Q cos(4 chi - 2 g) + ...])
    np.testing.assert_allclose(rows[5, 1:3], [0.5, 0.0], atol=1e-16)
    np.testing.assert_allclose(rows[8, 1:3], [0.0, 0.5], atol=1e-16)
    np.testing.assert_allclose(rows[7, 1:3], [-0.5, 0.0], atol=1e-16)
    np.testing.assert_allclose(rows[10, 1:3], [0.0, -0.5], atol=1e-16)
    # subset() carries the override
    sub = m.subset(np.array([1, 6, 9]))
    np.testing.assert_array_equal(sub.stokes_rows(), rows[[1, 6, 9]])
    np.testing.assert_array_equal(sub.gamma, m.gamma[[1, 6, 9]])
    # every detector on request: an unpolarised one's Q / U rows weigh nothing
    every = hwp.demodulated_detectors(d, polarized_only=False)
    assert every.n == 15 and np.all(every.stokes_rows()[[6, 11]] == 0)
    # stokes_rows() hands out a copy
    m.stokes_rows()[:] = 9.0
    np.testing.assert_array_equal(m.stokes_rows(), rows)


@pytest.mark.parametrize("gamma", [0.0, 0.7])
def test_the_reference_formula_recovers_q_and_u(gamma):
    """d = w_I I + w_I [Q cos(4 chi - 2 g) + U sin(4 chi - 2 g)] with slow I, Q, U far inside the pass band, I of order 5
    and Q, U of order 1e-3: in the interior y_t = w_I I, y_q = w_I (Q cos 2g - U sin 2g), y_u = w_I (Q sin 2g + U cos 2g)
    within the leakage bound 2 * 10^(-120 / 20) * max|x| (the design's stop band times the mixing's 2)."""
    fs, f, q, T = 200.0, 2.0, 8, 24000
    t = np.arange(T) / fs
    chi = hwp.HWP(f, phase=0.4).angle(t)
    c = hwp.carrier(chi)
    I = 5 + 0.5 * np.sin(2 * np.pi * 0.05 * t)  # noqa: E741
    Q = 2e-3 * np.cos(2 * np.pi * 0.11 * t + 0.3)
    U = -1e-3 * np.sin(2 * np.pi * 0.07 * t)
    w = mueller_row(np.array([gamma]))[0, 0]
    d = (w * I + w * (Q * np.cos(4 * chi - 2 * gamma) + U * np.sin(4 * chi - 2 * gamma)))[None]
    h = hwp.design_taps(fs, f)
    y_t, y_q, y_u, _, _ = ref.demodulate(d, c, q, h, h)
    H = (h.size - 1) // 2
    j = np.arange(y_t.shape[1])
    inner = (j * q >= H) & (j * q < T - H)
    assert inner.sum() > 1000
    pick = slice(None, None, q)
    bound = 2 * 10 ** (-120 / 20) * np.abs(d).max()
    errs = [np.abs(y_t[0] - (w * I)[pick])[inner].max(),
            np.abs(y_q[0] - (w * (Q * np.cos(2 * gamma) - U * np.sin(2 * gamma)))[pick])[inner].max(),
            np.abs(y_u[0] - (w * (Q * np.sin(2 * gamma) + U * np.cos(2 * gamma)))[pick])[inner].max()]
    print(f"gamma {gamma}: |y - expected| T {errs[0]:.2e} Q {errs[1]:.2e} U {errs[2]:.2e}, bound {bound:.2e}")
    # (the slow series themselves lose a little at the pass band's far end: 0.11 Hz is 0.11 / 1 of pass_edge f_hwp)
    assert max(errs) <= bound


def test_harmonic_templates():
    chi = np.linspace(0, 20, 501)
    B = hwp.harmonic_templates(chi, (1, 4))
    assert B.shape == (4, 501) and B.dtype == np.float32
    np.testing.assert_array_equal(B, np.stack([np.cos(chi), np.sin(chi), np.cos(4 * chi), np.sin(4 * chi)]).astype(np.float32))
    for bad in ((), (0,), (1, 1), (1.5,)):
        with pytest.raises(ValueError):
            hwp.harmonic_templates(chi, bad)


def test_demodulate_refuses_on_the_host(monkeypatch):
    """Everything mrx_tod_demodulate refuses raises ValueError on the host: no context is made and no entry is called."""
    import torch

    from maria_amd import _lib

    def no_context(*a, **k):
        raise AssertionError("a device context was made")

    monkeypatch.setattr(_lib, "Context", no_context)
    x = torch.zeros((4, 300), dtype=torch.float32)
    c = np.zeros((300, 2))
    h = np.ones(41) / 41
    good = dict(x=x, carrier=c, q=4, taps_p=h)
    bad = {
        "no taps": dict(good, taps_p=None),
        "q 1": dict(good, q=1),
        "q 33": dict(good, q=33),
        "q 2.5": dict(good, q=2.5),
        "even taps": dict(good, taps_p=np.ones(40)),
        "1027 taps": dict(good, taps_p=np.ones(1027)),
        "nan taps": dict(good, taps_p=np.full(41, np.nan)),
        "taps of two counts": dict(good, taps_t=np.ones(39)),
        "a truncated sum <= 0": dict(good, taps_p=np.r_[-np.ones(20), 0.5, np.ones(20)]),
        "float64 x": dict(good, x=x.double()),
        "1-d x": dict(good, x=x[0]),
        "strided x": dict(good, x=x[:, ::2]),
        "carrier of T - 1": dict(good, carrier=c[:-1]),
        "float32 carrier": dict(good, carrier=c.astype(np.float32)),
        "out of two": dict(good, out=(torch.zeros((4, 75)), torch.zeros((4, 75)))),
        "out with y_t without want_t": dict(good, want_t=False, out=(torch.zeros((4, 75)),) * 3),
        "out of the wrong shape": dict(good, out=(torch.zeros((4, 75)), torch.zeros((4, 75)), torch.zeros((4, 74)))),
        "out twice the same": dict(good, out=(torch.zeros((4, 75)),) + (torch.zeros((4, 75)),) * 2),
        "out of two pitches": dict(good, out=(torch.zeros((4, 75)), torch.zeros((4, 75)), torch.zeros((4, 80))[:, :75])),
        "out on x": dict(good, x=x[:, :75 * 4], carrier=c, out=(x[:, :75], torch.zeros((4, 75)), torch.zeros((4, 75)))),
        "a host tensor": good,  # the last refusal
    }
    for name, kw in bad.items():
        with pytest.raises(ValueError):
            hwp.demodulate(**kw)
            pytest.fail(name)
    z = torch.zeros((4, 300), dtype=torch.float32)
    for name, kw in {"two pitches": dict(s_i=z, s_c=z.clone(), s_s=torch.zeros((4, 304))[:, :300]),
                     "out is s_c": dict(s_i=z, s_c=z.clone(), s_s=z.clone(), out="s_c"),
                     "float64": dict(s_i=z, s_c=z.double(), s_s=z.clone()),
                     "a host tensor": dict(s_i=z, s_c=z.clone(), s_s=z.clone())}.items():
        if kw.get("out") == "s_c":
            kw["out"] = kw["s_c"]
        with pytest.raises(ValueError):
            hwp.modulate(carrier=c, **kw)
            pytest.fail(name)
