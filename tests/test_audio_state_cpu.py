"""CPU checks of the inputs and references the carried-state GPU tests rest on (tests/audio_state_cases.py): no GPU needed.

* the numpy f64 K-weighting impulse reference agrees with the oracle meter on every impulse case;
* the true-peak edge signals decide the oracle's true peak inside the event (the floor alone reads at least 20 dB lower) and
  are inputs on which a lost history WOULD show: zeroing the `delay` frames in front of the cut changes the oracle's reading;
* the float32 restatement of the partitioned convolution agrees with the f64 time-domain renderer within the figures the
  device bound is derived from, and those figures are the ones tabulated."""
import numpy as np
import pytest

import audio_state_cases as A


@pytest.mark.parametrize("sizes,pos", A.IMPULSE_CASES)
def test_kweighting_impulse_reference_agrees_with_the_oracle(oracle, sizes, pos):
    ref = oracle.EbuR128(3, A.IMPULSE_RATE, 63, A.IMPULSE_CLASSES)
    b, a = ref.filter_coeffs()
    for part in A.split(A.impulse_stream(sizes, pos), sizes):
        ref.add_frames(part.reshape(-1))
    exp = A.impulse_momentary(b, a, sizes, pos)
    assert abs(ref.loudness_momentary() - exp) <= 1e-9, (ref.loudness_momentary(), exp)
    # the reading is made of the impulse response: carried values that slip by one position at a cut shortly after the impulse
    # move it far outside the tolerance
    n = sum(sizes) - pos
    for at in (1, 2, 5):
        slipped = A.kweight_impulse_energy(b, a, n, shift_state_at=at)
        assert abs(10.0 * np.log10(slipped / A.kweight_impulse_energy(b, a, n))) > 1e-3


def _oracle_tp(oracle, rate, x, mode=63):
    m = oracle.EbuR128(x.shape[1], rate, mode)
    m.add_frames(np.ascontiguousarray(x).reshape(-1))
    return [m.true_peak(c) for c in range(x.shape[1])], [m.sample_peak(c) for c in range(x.shape[1])]


@pytest.mark.parametrize("rate", A.EB_RATES)
def test_truepeak_edge_signals_are_decided_at_the_event(oracle, rate):
    ch = 4
    x, floor, where = A.tp_stream(rate, ch)
    tp, sp = _oracle_tp(oracle, rate, x.astype(np.float32))
    tpf, _ = _oracle_tp(oracle, rate, floor.astype(np.float32))
    for c in range(ch):
        assert 20.0 * np.log10(tp[c] / tpf[c]) >= 20.0          # the floor's own maximum cannot pass for the event's
        if A.eb_delay(rate):
            assert tp[c] > sp[c] * 1.02                          # an inter-sample over: the interpolated peak, not a sample, decides
        else:
            assert tp[c] == sp[c]                                # 192 kHz: no interpolator
    d = A.eb_delay(rate)
    if not d:
        return
    for cut in A.tp_cuts(rate):
        lost = x.copy()
        lost[cut - d:cut] = 0.0                                  # what a zeroed history would make of the stream
        tpl, _ = _oracle_tp(oracle, rate, lost.astype(np.float32))
        assert any(tpl[c] != tp[c] for c in range(ch)), cut
        early = x.copy()
        early[cut - d:cut] = x[cut - d - 1:cut - 1]              # a history taken one frame early
        tpe, _ = _oracle_tp(oracle, rate, early.astype(np.float32))
        assert any(tpe[c] != tp[c] for c in range(ch)), cut


def test_truepeak_integer_minimum_maps_to_full_scale(oracle):
    x, _, where = A.tp_stream(48000, 2)
    for dtype in (np.int16, np.int32):
        y = A.tp_format(x, where, dtype)
        assert y[where[0][0], 0] == np.iinfo(dtype).min
        m = oracle.EbuR128(2, 48000, 63)
        m.add_frames(y.reshape(-1))
        assert m.sample_peak(0) == 1.0 and m.true_peak(0) > 1.0


def test_fft32_is_a_float32_transform():
    rng = np.random.default_rng(4)
    for n in (16, 1024, 4096):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        X = A.fft32(x)
        assert X.dtype == np.complex64
        ref = np.fft.fft(x.astype(np.complex128))
        assert np.abs(X - ref).max() <= 2e-6 * np.abs(ref).max()
        back = A.fft32(X, inverse=True) / n
        assert np.abs(back - x).max() <= 2e-6 * np.abs(x).max()


@pytest.mark.parametrize("shape", A.SOFA_NEW_SHAPES, ids=["-".join(map(str, s)) for s in A.SOFA_NEW_SHAPES])
def test_float32_restatement_error_is_the_tabulated_one(oracle, shape):
    worst, scale = A.sofa_run(shape, A.SofaF32)
    fig, tab = worst / scale, A.SOFA_F32_ERR[shape]
    assert fig <= 2.0 * tab and fig >= 0.5 * tab, (shape, fig, tab)


def test_float32_restatement_places_the_taps(oracle):
    """the restatement itself reproduces integer taps at the right sample and ear (it sets a bound: it must be right)"""
    C, L, P, B = 1, 40, 16, 64
    r = A.SofaF32(C, L, P, B)
    l, rr = np.arange(1, L + 1, dtype=np.float32), np.arange(101, 101 + L, dtype=np.float32)
    r.set_filter(0, l, rr)
    x = np.zeros((B, 1), np.float32)
    x[17, 0] = 1.0
    a = r.process_block(x, [1.0])
    exp = np.zeros((B, 2))
    exp[17:17 + L, 0], exp[17:17 + L, 1] = l, rr
    assert (np.round(a) == exp).all() and np.abs(a - exp).max() < 1e-3


def test_hrir_taps_follow_the_sphere_layout(oracle, synth):
    import os
    mesh = open(os.path.join(os.path.dirname(__file__), "golden", "test.hrir"), "rb").read()
    data = synth.hrir_sphere_bytes(mesh, 24)
    sphere = oracle.HrirSphere(data, 44100)
    pos = np.array([[0.9, 0.1, 0.3]], np.float32)
    face, uvw = sphere.sample(pos[0])
    assert face >= 0
    left, right = A.hrir_taps(data, face, uvw)
    ex = oracle.HrtfExact(sphere, 1, 1, 32)
    x = np.zeros((32, 1), np.float32)
    x[3, 0] = 1.0
    y = ex.process_block(x, pos, np.array([0.5], np.float32)).reshape(32, 2)
    exp = np.zeros((32, 2))
    exp[3:27, 0], exp[3:27, 1] = 0.5 * left, 0.5 * right
    assert np.abs(y - exp).max() <= 1e-6
    assert np.abs(y[:, ::-1] - exp).max() > 1e-2      # the ears differ: a swap is not a rounding matter
