"""agingradio on the GPU: mi355_agingradio_* and the agingradio audio-group kind against the independent restatement
(tests/agingradio_restate.py, DESIGN §4.9: parity unpinned), bit for bit, and the element mirror's property rules
(audio/audiofx/src/agingradio/imp.rs)."""
import threading

import numpy as np
import pytest

import agingradio_restate as R
import mi355fx
from mi355fx.elements import FLOW_NOT_NEGOTIATED, FLOW_OK, Element

pytestmark = pytest.mark.gpu

SETTINGS = {
    "defaults": {},
    "noise": dict(white_noise_ampl=0.3),
    "ampl1": dict(white_noise_ampl=1.0),
    "clicks_1e-5": dict(clicks_prob=1e-5),
    "clicks_half": dict(clicks_prob=0.5),
    "clicks_all": dict(clicks_prob=1.0),
    "lowpass": dict(lowpass_freq=2000),
    "lowpass_1hz": dict(lowpass_freq=1),
    "bits4": dict(bits_to_quantize=4.0),
    "bits_half": dict(bits_to_quantize=0.5),
    "bits64": dict(bits_to_quantize=64.0),
    "cubic1": dict(cubic_curve_distortion=0.7, cubic_curve_passes=1),
    "cubic50": dict(cubic_curve_distortion=1.0, cubic_curve_passes=50),
    "passes0": dict(cubic_curve_distortion=1.0, cubic_curve_passes=0),
}


def _settings(name):
    """'defaults' is the element's defaults; every other entry is that knob alone on top of everything off."""
    return dict(R.DEFAULTS) if name == "defaults" else dict(R.OFF, **SETTINGS[name])


def _signal(frames, channels, dtype, seed=0, special=False):
    rng = np.random.default_rng(seed + 31 * channels + frames)
    x = rng.uniform(-1.2, 1.2, frames * channels)
    if special and x.size >= 16:
        x[:8] = [np.nan, np.inf, -np.inf, 5e-324, -2.5e-310, 1e300, -40.0, 7.5]
        if dtype == np.float32:
            x[3:5] = [1e-40, -3e-45]
            x[5] = 3e38
    return x.astype(dtype)


def _check(ctx, x, channels, rate, s, seed, device=False):
    want = R.AgingRadio(channels, rate, s["lowpass_freq"], seed).process(x, **s)
    ctx.agingradio_setup(channels, rate, s["lowpass_freq"], seed)
    got = x.copy()
    if device:
        d = ctx.alloc(max(got.nbytes, 16))
        try:
            if got.nbytes:
                ctx.h2d(d, got)
            ctx.agingradio_process_device(d, x.size // channels, got.dtype == np.float64, s)
            ctx.synchronize()
            if got.nbytes:
                ctx.d2h(got, d)
        finally:
            ctx.free(d)
    else:
        ctx.agingradio_process(got, channels, s)
    assert got.tobytes() == want.tobytes(), (channels, x.size // channels, x.dtype, s, int(np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))[0]))
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("channels", [1, 2, 6, 65])
def test_defaults_over_buffer_sizes(ctx, dtype, channels):
    for frames in (0, 1, 2, 479, 480, 48000):
        _check(ctx, _signal(frames, channels, dtype), channels, 48000, _settings("defaults"), seed=0xC0FFEE + frames)


@pytest.mark.parametrize("name", sorted(SETTINGS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_knob(ctx, name, dtype):
    s = _settings(name)
    for channels, frames in ((2, 4801), (65, 479), (1, 960)):
        _check(ctx, _signal(frames, channels, dtype, special=True), channels, 48000, s, seed=1234567 + channels)


@pytest.mark.parametrize("rate", [8000, 192000])
def test_lowpass_22k_at_extreme_rates(ctx, rate):
    for dtype in (np.float32, np.float64):
        s = dict(R.DEFAULTS, lowpass_freq=22000)
        _check(ctx, _signal(3001, 2, dtype, special=True), 2, rate, s, seed=rate)
        _check(ctx, _signal(3001, 6, dtype), 6, rate, dict(R.OFF, lowpass_freq=22000), seed=rate + 1)


def test_far_outside_unit_range_and_specials(ctx):
    for dtype in (np.float32, np.float64):
        x = _signal(2000, 2, dtype, special=True) * dtype(1e3)
        _check(ctx, x, 2, 44100, dict(R.DEFAULTS, clicks_prob=0.01), seed=9)
        _check(ctx, x, 2, 44100, dict(R.DEFAULTS, lowpass_freq=0, clicks_prob=0.01), seed=9)


def test_host_and_device_entry_points_agree(ctx):
    for dtype in (np.float32, np.float64):
        for lp in (0, 2000):
            s = dict(R.DEFAULTS, lowpass_freq=lp, clicks_prob=0.02)
            x = _signal(4097, 6, dtype)
            a = _check(ctx, x, 6, 48000, s, seed=77, device=False)
            b = _check(ctx, x, 6, 48000, s, seed=77, device=True)
            assert a.tobytes() == b.tobytes()


def test_ragged_buffers_carry_state_and_reset_restarts(ctx):
    for lp in (0, 2000):
        s = dict(R.DEFAULTS, lowpass_freq=lp, clicks_prob=0.01)
        ref = R.AgingRadio(2, 48000, lp, 4242)
        ctx.agingradio_setup(2, 48000, lp, 4242)
        for frames in (480, 7, 1, 0, 2, 481, 9000, 33):   # odd buffers: each leaves its last frame alone
            for dtype in (np.float32, np.float64):
                x = _signal(frames, 2, dtype, seed=frames)
                want = ref.process(x, **s)
                ctx.agingradio_process(x, 2, s)
                assert x.tobytes() == want.tobytes(), (lp, frames)
                y, k = ctx.agingradio_state(2)
                assert k == ref.k
                if lp:
                    assert y.tobytes() == ref.y.tobytes()
        # a new setup restarts the filters and the pair counter
        ctx.agingradio_setup(2, 48000, lp, 4242)
        assert ctx.agingradio_state(2)[1] == 0 and np.all(ctx.agingradio_state(2)[0] == 0)
        _check(ctx, _signal(480, 2, np.float32), 2, 48000, s, seed=4242)
        # stop drops the state: process is NotNegotiated's status until the next setup
        ctx.agingradio_reset()
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.agingradio_process(_signal(4, 2, np.float32), 2, s)
        assert e.value.status == mi355fx.ERR_NOT_CONFIGURED


def test_seeds(ctx):
    x = _signal(960, 2, np.float64)
    s = dict(R.DEFAULTS, clicks_prob=0.01)
    a = _check(ctx, x, 2, 48000, s, seed=1)
    b = _check(ctx, x, 2, 48000, s, seed=1)
    c = _check(ctx, x, 2, 48000, s, seed=2)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()


def test_validation(ctx):
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.agingradio_process(np.zeros(4, np.float32), 2, {})
    assert e.value.status == mi355fx.ERR_NOT_CONFIGURED
    for ch, rate in ((0, 48000), (2, 0)):
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.agingradio_setup(ch, rate, 2000, 1)
        assert e.value.status == mi355fx.ERR_INVALID_ARG


def _member_plan(m):
    rng = np.random.default_rng(m)
    channels = [1, 2, 6, 65, 2][m % 5]
    rate = [48000, 44100, 8000, 192000][m % 4]
    lp = [2000, 0, 1, 22000][(m // 2) % 4]
    names = sorted(SETTINGS)
    s = dict(_settings(names[m % len(names)]), lowpass_freq=lp)
    dtype = np.float32 if m % 3 else np.float64
    sizes = [int(v) for v in rng.integers(0, 700, 5)]
    return channels, rate, lp, 1000 + 17 * m, s, dtype, sizes


@pytest.mark.parametrize("n_members", [1, 7, 32])
def test_group_members_equal_their_own_context(mi355lib, n_members):
    g = mi355fx.AudioGroup("agingradio", n_members)
    g.set_linger(2000)
    try:
        plans = [_member_plan(m) for m in range(n_members)]
        for m, (ch, rate, lp, seed, s, dtype, sizes) in enumerate(plans):
            g.agingradio_setup(m, ch, rate, lp, seed)
        results, errors = {}, []
        device = {m: (m % 4 == 1) for m in range(n_members)}
        late, gone = n_members - 1, (n_members - 2 if n_members > 2 else None)

        def member(m):
            try:
                ch, rate, lp, seed, s, dtype, sizes = plans[m]
                ctx = mi355fx.Context(0)
                outs = []
                for i, frames in enumerate(sizes):
                    if m == gone and i == 2:
                        g.detach(m)
                        break
                    if m == late and i == 0:
                        threading.Event().wait(0.01)
                    x = _signal(frames, ch, dtype, seed=m * 100 + i)
                    if device[m] and x.nbytes:
                        d = ctx.alloc(x.nbytes)
                        ctx.h2d(d, x)
                        g.wait(g.submit_agingradio(m, d, s, frames=frames, is_f64=dtype == np.float64))
                        ctx.d2h(x, d)
                        ctx.free(d)
                    else:
                        g.wait(g.submit_agingradio(m, x, s, channels=ch))
                    outs.append(x)
                results[m] = (outs, g.agingradio_state(m, ch))
                ctx.close()
            except Exception as e:   # noqa: BLE001 - reported below
                errors.append((m, repr(e)))

        ts = [threading.Thread(target=member, args=(m,)) for m in range(n_members)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not errors, errors
        ctx = mi355fx.Context(0)
        for m, (ch, rate, lp, seed, s, dtype, sizes) in enumerate(plans):
            outs, (y, k) = results[m]
            ctx.agingradio_setup(ch, rate, lp, seed)
            for i, got in enumerate(outs):
                x = _signal(sizes[i], ch, dtype, seed=m * 100 + i)
                ctx.agingradio_process(x, ch, s)
                assert got.tobytes() == x.tobytes(), (m, i)
            y0, k0 = ctx.agingradio_state(ch)
            assert k == k0 and y.tobytes() == y0.tobytes(), m
        ctx.close()
    finally:
        g.close()


def test_group_errors(mi355lib):
    L = mi355lib
    g = mi355fx.AudioGroup("agingradio", 2)
    e = mi355fx.AudioGroup("echo", 2, ring_len=16)
    try:
        with pytest.raises(mi355fx.Mi355Error) as ex:   # a submit before the member's setup
            g.submit_agingradio(0, np.zeros(8, np.float32), {}, channels=2)
        assert ex.value.status == mi355fx.ERR_NOT_CONFIGURED
        for member in (-1, 2):   # bad member
            with pytest.raises(mi355fx.Mi355Error) as ex:
                g.agingradio_setup(member, 2, 48000, 2000, 1)
            assert ex.value.status == mi355fx.ERR_INVALID_ARG
            with pytest.raises(mi355fx.Mi355Error) as ex:
                g.agingradio_state(member, 2)
            assert ex.value.status == mi355fx.ERR_INVALID_ARG
        with pytest.raises(mi355fx.Mi355Error) as ex:
            g.agingradio_setup(0, 0, 48000, 2000, 1)
        assert ex.value.status == mi355fx.ERR_INVALID_ARG
        # wrong kind: an echo group takes no agingradio member, an agingradio group no echo buffer
        st = mi355fx.AgingRadioSettings.of({})
        assert L.mi355_agroup_agingradio_setup(e.h, 0, 2, 48000, 2000, 1) == mi355fx.ERR_INVALID_ARG
        assert b"another element kind" in L.mi355_agroup_last_error(e.h)
        assert L.mi355_agroup_submit_agingradio(e.h, 0, None, 0, 0, mi355fx.C.byref(st), 1, None) == mi355fx.ERR_INVALID_ARG
        with pytest.raises(mi355fx.Mi355Error) as ex:
            g.submit_echo(0, np.zeros(4, np.float32), 0, 0.5, 0.0)
        assert ex.value.status == mi355fx.ERR_INVALID_ARG
    finally:
        g.close()
        e.close()


def test_shared_group_hands_out_members(mi355lib):
    a = mi355fx.AudioGroup("agingradio", 2, shared=True)
    b = mi355fx.AudioGroup("agingradio", 2, shared=True)
    try:
        assert a.h == b.h and {a.member, b.member} == {0, 1}
    finally:
        for x in (a, b):
            x.close()


def test_element_property_rules_and_transform_ip(ctx):
    el = Element.agingradio()
    props = el.properties()
    assert set(props) == {"white-noise-ampl", "clicks-prob", "lowpass-freq", "bits-to-quantize", "cubic-curve-distortion", "cubic-curve-passes"}
    assert all(p["mutable"] == "ready" for p in props.values())
    assert el.type_name == "GstRsAgingRadio" and el.klass == "Filter/Effect/Audio"
    assert el.get_property("clicks-prob") == float(np.float32(1e-5)) and el.get_property("lowpass-freq") == 2000
    assert not el.set_property("white-noise-ampl", 1.5) and not el.set_property("lowpass-freq", 22001)
    x = _signal(480, 2, np.float32)
    assert el.agingradio_transform_ip(x.copy()) == FLOW_NOT_NEGOTIATED
    assert el.set_property("white-noise-ampl", 0.25) and el.set_property("lowpass-freq", 1000)
    assert el.start() and el.agingradio_setup(48000, 2, False, seed=55)
    # white-noise-ampl is ignored while there is a state; the others are written at once, lowpass-freq counts at the next setup
    assert el.set_property("white-noise-ampl", 0.5) and el.get_property("white-noise-ampl") == 0.25
    assert el.set_property("bits-to-quantize", 6.0) and el.set_property("lowpass-freq", 3000)
    s = dict(R.DEFAULTS, white_noise_ampl=0.25, bits_to_quantize=6.0, lowpass_freq=1000)
    want = R.AgingRadio(2, 48000, 1000, 55).process(x, **s)
    got = x.copy()
    assert el.agingradio_transform_ip(got) == FLOW_OK and got.tobytes() == want.tobytes()
    # the ABI with the same seed and settings gives the same buffer
    y = x.copy()
    ctx.agingradio_setup(2, 48000, 1000, 55)
    ctx.agingradio_process(y, 2, s)
    assert y.tobytes() == got.tobytes()
    assert el.stop() and el.agingradio_transform_ip(x.copy()) == FLOW_NOT_NEGOTIATED
    assert el.set_property("white-noise-ampl", 0.5) and el.get_property("white-noise-ampl") == 0.5
    el.close()
