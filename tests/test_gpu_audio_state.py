"""State the audio kernels carry across the cuts they make, tested where it is decided: events on the buffer edge, impulses at the
chunk boundary, steps on the ring wrap, impulses through the partitioned convolvers, the device entry points.

ebur128level  peaks must EQUAL the oracle's after every buffer and equal the same stream fed as one buffer (the tap order of
              an interpolated sample does not depend on where a buffer ends); loudness within the meter file's 1e-9 LU.
sofalizer     against oracle.SofaRenderer (f64 time domain) with the rule of tests/test_gpu_sofa.py, 2e-6 * scale * max(1, L // 64),
              at the small shapes used here; integer taps must come back at the right sample of the right ear.
hrtfrender    impulse against the blend of the sphere's own HRIRs; step bounds and short blocks against the f64 evaluation.
Signals and references: tests/audio_state_cases.py (checked on the CPU in tests/test_audio_state_cpu.py)."""
import os

import numpy as np
import pytest

import audio_state_cases as A

pytestmark = pytest.mark.gpu

EB_TOL = 1e-9          # LU, as tests/test_gpu_ebur128.py
SOFA_TOL = 2e-6        # as tests/test_gpu_sofa.py
HRTF_TOL_EXACT = 2e-5  # as tests/test_gpu_hrtf.py
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "test.hrir")


def _close(a, b):
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= EB_TOL


def _peaks(m, ch, dev):
    if dev:
        return [m.ebur128_true_peak(c) for c in range(ch)], [m.ebur128_sample_peak(c) for c in range(ch)]
    return [m.true_peak(c) for c in range(ch)], [m.sample_peak(c) for c in range(ch)]


def _feed(m, part, planar, dev):
    data = np.ascontiguousarray(part.T) if planar else np.ascontiguousarray(part).reshape(-1)
    if dev:
        m.ebur128_add_frames(data, planar=planar)
    else:
        m.add_frames(data, planar=planar)


@pytest.fixture()
def ctx2(mi355lib):
    import mi355fx
    c = mi355fx.Context(0)
    yield c
    c.close()


def _check_split(ctx, ctx2, oracle, rate, x, sizes, planar=False):
    """the stream in buffers of `sizes`: peaks equal to the oracle's after every buffer, and at the end equal to one buffer"""
    ch = x.shape[1]
    ctx.ebur128_setup(ch, rate, 63, [1] * ch)
    ref = oracle.EbuR128(ch, rate, 63, [1] * ch)
    for part in A.split(x, sizes):
        _feed(ctx, part, planar, True)
        _feed(ref, part, planar, False)
        assert _peaks(ctx, ch, True) == _peaks(ref, ch, False), (rate, sizes)
    ctx2.ebur128_setup(ch, rate, 63, [1] * ch)
    _feed(ctx2, x, planar, True)
    assert _peaks(ctx, ch, True) == _peaks(ctx2, ch, True), (rate, sizes)


@pytest.mark.parametrize("rate", A.EB_RATES)
def test_true_peak_event_on_the_buffer_edge(ctx, ctx2, oracle, rate):
    """the cut at every offset from -delay to +delay around four staggered inter-sample overs: the interpolated peak draws on
    the history kept from the previous buffer"""
    x, _, where = A.tp_stream(rate, 4)
    x = A.tp_format(x, where, np.float32)
    for cut in A.tp_cuts(rate):
        _check_split(ctx, ctx2, oracle, rate, x, [cut, len(x) - cut])


@pytest.mark.parametrize("rate", A.EB_RATES)
def test_true_peak_through_runs_of_short_buffers(ctx, ctx2, oracle, rate):
    """runs of 1, 2, delay - 1, delay, delay + 1 frame buffers up to and across the events: the history update for buffers
    shorter than the history (older samples shift down) and just above it"""
    x, _, where = A.tp_stream(rate, 4)
    x = A.tp_format(x, where, np.float32)
    for sizes in A.tp_short_schedules(rate, len(x)):
        _check_split(ctx, ctx2, oracle, rate, x, sizes)


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
@pytest.mark.parametrize("planar", [False, True])
def test_true_peak_edge_in_every_format_and_layout(ctx, ctx2, oracle, dtype, planar):
    """the eight format x layout combinations; the integer formats carry their minimum (exactly -1.0) in the event"""
    rate = 48000
    x, _, where = A.tp_stream(rate, 4)
    x = A.tp_format(x, where, dtype)
    for cut in A.tp_cuts(rate)[::2]:
        _check_split(ctx, ctx2, oracle, rate, x, [cut, len(x) - cut], planar)
    d = A.eb_delay(rate)
    _check_split(ctx, ctx2, oracle, rate, x, A.tp_short_schedules(rate, len(x))[2], planar)
    _check_split(ctx, ctx2, oracle, rate, x, [A.EB_LEAD - d, 1, 2, d - 1, 1, len(x) - A.EB_LEAD - 3], planar)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("channels", [1, 2, 6, 64])
def test_sample_peak_in_the_first_and_last_frame(ctx, oracle, channels, planar):
    """every channel's peak sits in the first or the last frame of a buffer (the last channel included, 64 channels = the setup
    limit and the 130 KiB LDS request of the filter kernel); buffers of 1, 255, 256, 257 and 600 frames"""
    rate = 48000
    classes = [1 if c % 5 else 0 for c in range(channels)] if channels > 1 else [1]
    ctx.ebur128_setup(channels, rate, 1 | 16, classes)
    ref = oracle.EbuR128(channels, rate, 1 | 16, classes)
    rng = np.random.default_rng(channels)
    want = np.zeros(channels)
    for k, n in enumerate([300, 1, 255, 256, 257, 600]):
        x = A.FLOOR * rng.uniform(-1, 1, (n, channels))
        for c in range(channels):
            if (c + k) % 3 == 0 or c == channels - 1:
                v = (0.1 + 0.1 * k + 0.001 * c) * (-1.0) ** c
                x[0 if (c + k) % 2 else n - 1, c] = v
        x = x.astype(np.float32)
        want = np.maximum(want, np.abs(x.astype(np.float64)).max(axis=0))
        _feed(ctx, x, planar, True)
        _feed(ref, x, planar, False)
        got = [ctx.ebur128_sample_peak(c) for c in range(channels)]
        assert got == [ref.sample_peak(c) for c in range(channels)]
        assert got == list(want)
        assert _close(ctx.ebur128_loudness_momentary(), ref.loudness_momentary())


@pytest.mark.parametrize("sizes,pos", A.IMPULSE_CASES)
def test_filter_state_across_chunks_and_calls_impulse(ctx, oracle, sizes, pos):
    """a unit impulse at frame 255 / 256 / 257 of a buffer, in its last frame, in a 1-frame buffer: the momentary reading IS the
    squared K-weighting impulse response, so carried values that slip by one position change it grossly. Against the oracle
    under the same splits and against the numpy f64 recurrence; the class-0 channel between the used ones must not count."""
    ctx.ebur128_setup(3, A.IMPULSE_RATE, 63, A.IMPULSE_CLASSES)
    ref = oracle.EbuR128(3, A.IMPULSE_RATE, 63, A.IMPULSE_CLASSES)
    for part in A.split(A.impulse_stream(sizes, pos), sizes):
        _feed(ctx, part, False, True)
        _feed(ref, part, False, False)
        assert _close(ctx.ebur128_loudness_momentary(), ref.loudness_momentary())
        assert _close(ctx.ebur128_loudness_shortterm(), ref.loudness_shortterm())
    b, a = ref.filter_coeffs()
    got, exp = ctx.ebur128_loudness_momentary(), A.impulse_momentary(b, a, sizes, pos)
    assert abs(got - exp) <= EB_TOL, (got, exp)
    assert _peaks(ctx, 3, True) == _peaks(ref, 3, False)


@pytest.mark.parametrize("chunk", [0, 1600, 257])
def test_filter_state_that_underflows_in_silence(ctx, oracle, chunk):
    """a burst, silence long enough for the filter state to underflow, a second burst; fed in one buffer and in many. libebur128
    flushes denormal state at the end of each call, so the two feeds may legitimately differ in the last bits: each is compared
    with the oracle under identical splits only."""
    rate, ch = 16000, 2
    rng = np.random.default_rng(8)
    burst = 0.3 * rng.standard_normal((1600, ch))
    x = np.concatenate([burst, np.zeros((4 * rate, ch)), 0.5 * burst[:800]])
    sizes = [len(x)] if chunk == 0 else [chunk] * (len(x) // chunk) + ([len(x) % chunk] if len(x) % chunk else [])
    ctx.ebur128_setup(ch, rate, 63, [1, 1])
    ref = oracle.EbuR128(ch, rate, 63, [1, 1])
    for i, part in enumerate(A.split(x, sizes)):
        _feed(ctx, part, False, True)
        _feed(ref, part, False, False)
        if i % 16 == 0 or i == len(sizes) - 1:
            assert _close(ctx.ebur128_loudness_momentary(), ref.loudness_momentary())
    assert _close(ctx.ebur128_loudness_shortterm(), ref.loudness_shortterm())
    assert _close(ctx.ebur128_loudness_global(), ref.loudness_global())
    assert _peaks(ctx, ch, True) == _peaks(ref, ch, False)


@pytest.mark.parametrize("rate", [44100, 22050, 11025])
def test_level_step_across_the_ring_wrap(ctx, oracle, rate):
    """a 20 dB step placed so that the short-term window straddles the wrap point of the 3 s ring, read every 100 ms for more
    than one turn of the ring past the step. 44100 and 22050 Hz divide into whole 100 ms blocks; at 11025 Hz the ring is rounded
    up (33075 -> 33090 frames = 30 x 1103), which is where the rounding bites."""
    ch, s100 = 2, (rate + 5) // 10
    n = 64 * s100
    t = np.arange(n) / rate
    level = np.where(np.arange(n) < 28 * s100 + s100 // 3, 0.01, 0.1)
    x = (level * np.sin(2 * np.pi * 997.0 * t))[:, None] * np.array([1.0, 0.7])[None, :]
    x = x.astype(np.float32)
    ctx.ebur128_setup(ch, rate, 63)
    ref = oracle.EbuR128(ch, rate, 63)
    sizes = [25 * s100 + 123] + [s100] * 37
    sizes.append(n - sum(sizes))
    for part in A.split(x, sizes):
        _feed(ctx, part, False, True)
        _feed(ref, part, False, False)
        assert _close(ctx.ebur128_loudness_momentary(), ref.loudness_momentary())
        assert _close(ctx.ebur128_loudness_shortterm(), ref.loudness_shortterm())
    assert _close(ctx.ebur128_loudness_global(), ref.loudness_global())
    assert _close(ctx.ebur128_loudness_range(), ref.loudness_range())


def test_batch_true_peak_edge_equals_separate_meters(ctx):
    """five streams, the events at a different offset from the common cut in each: bit for bit what five single meters read"""
    import mi355fx
    rate, ch, S = 48000, 2, 5
    x, _, where = A.tp_stream(rate, ch)
    x = x.astype(np.float32)
    data = np.stack([np.roll(x, 5 * s - 11, axis=0) for s in range(S)])
    cut = A.EB_LEAD - 8
    singles = []
    for s in range(S):
        with mi355fx.Context(0) as c1:
            c1.ebur128_setup(ch, rate, 63)
            rows = []
            for part in (data[s, :cut], data[s, cut:cut + 5], data[s, cut + 5:]):
                c1.ebur128_add_frames(np.ascontiguousarray(part).reshape(-1))
                rows.append(_peaks(c1, ch, True))
            singles.append(rows)
    ctx.ebur128_setup_batch(S, ch, rate, 63)
    for k, part in enumerate((data[:, :cut], data[:, cut:cut + 5], data[:, cut + 5:])):
        ctx.ebur128_add_frames_batch(part)
        tp, sp = ctx.ebur128_peak_batch(True), ctx.ebur128_peak_batch(False)
        for s in range(S):
            assert (list(tp[s]), list(sp[s])) == singles[s][k], (s, k)


# ------------------------------------------------------------------ sofalizer

def _sofa_pair(ctx, oracle, C, L, P, B, flt, delays=None):
    ref = oracle.SofaRenderer(C, L, B)
    ctx.sofa_setup(C, L, P, B)
    for c, (l, r) in enumerate(flt):
        d = delays[c] if delays else (0, 0)
        ctx.sofa_set_filter(c, l, r, *d)
        ref.set_filter(c, l, r, *d)
    return ref


def _sofa_tol(L, exp):
    return SOFA_TOL * max(1.0, float(np.abs(exp).max())) * max(1, L // 64)


def test_sofalizer_swap_before_every_block(ctx, oracle):
    """K = 5 delay-line slots, 3 sub-blocks per block: the block start visits every slot; filters of several channels at once are
    replaced before EVERY block, back to the first set in between, with onset delays that cut all taps (delay >= L: that ear is
    silent) or all but one (delay == L - 1)"""
    C, L, P, B = 3, 80, 16, 48
    rng = np.random.default_rng(31)
    sets = [A.sofa_filters(rng, C, L) for _ in range(3)]
    ref = _sofa_pair(ctx, oracle, C, L, P, B, sets[0])
    g = np.array([1.0, 0.8, 0.6], np.float32)
    delays = [(0, 0), (L, 0), (L - 1, 3), (0, L + 7), (2, L - 1)]
    for blk in range(11):
        flt = sets[[1, 2, 0][blk % 3]]
        for c in ([0, 2], [1], [0, 1, 2])[blk % 3]:
            d = delays[(blk + c) % len(delays)]
            ctx.sofa_set_filter(c, flt[c][0], flt[c][1], *d)
            ref.set_filter(c, flt[c][0], flt[c][1], *d)
        x = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
        got, exp = ctx.sofa_process_block(x, g), ref.process_block(x, g)
        assert np.abs(got - exp).max() <= _sofa_tol(L, exp), blk


def test_sofalizer_all_taps_cut_is_silence(ctx, oracle):
    C, L, P, B = 1, 33, 16, 32
    rng = np.random.default_rng(2)
    l, r = A.sofa_filters(rng, 1, L)[0]
    ctx.sofa_setup(C, L, P, B)
    ctx.sofa_set_filter(0, l, r, L, L - 1)
    x = rng.standard_normal((B, 1)).astype(np.float32)
    outs = np.concatenate([ctx.sofa_process_block(x if k == 0 else np.zeros_like(x), [1.0]) for k in range(3)])
    assert (outs[:, 0] == 0).all()                                   # every left tap was pushed beyond the filter length
    exp = np.zeros(3 * B)
    exp[L - 1:L - 1 + B] = x[:, 0].astype(np.float64) * float(r[0])  # one right tap survives, L - 1 samples late
    assert np.abs(outs[:, 1] - exp).max() <= 1e-5


def test_sofalizer_dropped_channels_first_last_and_several(ctx, oracle):
    """what the element can do with ChannelProcessor::Drop: fixed per channel before the first block. The first, the last and a
    middle channel are dropped, each carrying a loud signal that must not reach the output; after the first block the flags are
    fixed (mi355_sofa_set_drop fails) until a reset."""
    import mi355fx
    C, L, P, B = 8, 70, 32, 64
    rng = np.random.default_rng(12)
    flt = A.sofa_filters(rng, C, L)
    dropped = (0, 4, C - 1)
    ref = oracle.SofaRenderer(C, L, B)
    ctx.sofa_setup(C, L, P, B)
    for c, (l, r) in enumerate(flt):
        if c in dropped:
            ctx.sofa_set_drop(c)
            ref.drop[c] = True
        else:
            ctx.sofa_set_filter(c, l, r)
            ref.set_filter(c, l, r)
    g = np.linspace(1.0, 0.5, C).astype(np.float32)
    for blk in range(4):
        x = (0.3 * rng.standard_normal((B, C))).astype(np.float32)
        for c in dropped:
            x[:, c] = 1000.0 * (1 + c)
        got, exp = ctx.sofa_process_block(x, g), ref.process_block(x, g)
        assert np.abs(got - exp).max() <= _sofa_tol(L, exp)
    for c, flag in ((0, False), (1, True)):
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.sofa_set_drop(c, flag)
        assert e.value.status == mi355fx.ERR_INVALID_ARG
    x = (0.3 * rng.standard_normal((B, C))).astype(np.float32)       # the refused calls changed nothing
    got, exp = ctx.sofa_process_block(x, g), ref.process_block(x, g)
    assert np.abs(got - exp).max() <= _sofa_tol(L, exp)
    ctx.sofa_reset()                                                 # history gone: the flags may be set again
    ref.reset()
    ctx.sofa_set_drop(0, False)
    ctx.sofa_set_filter(0, *flt[0])
    ref.drop[0] = False
    ref.set_filter(0, *flt[0])
    x[:, 0] = 0.25
    got, exp = ctx.sofa_process_block(x, g), ref.process_block(x, g)
    assert np.abs(got - exp).max() <= _sofa_tol(L, exp)


def test_sofalizer_reset_then_real_input_equals_a_fresh_renderer(ctx, ctx2, oracle):
    """reset in mid-run at a slot other than 0, then real input: bit for bit a fresh renderer with the same filters"""
    C, L, P, B = 2, 100, 16, 48      # K = 7, 3 sub-blocks per block
    rng = np.random.default_rng(77)
    flt = A.sofa_filters(rng, C, L)
    ref = _sofa_pair(ctx, oracle, C, L, P, B, flt)
    _sofa_pair(ctx2, oracle, C, L, P, B, flt)
    g = np.array([0.9, 0.7], np.float32)
    for _ in range(3):
        ctx.sofa_process_block(rng.standard_normal((B, C)).astype(np.float32), g)
    ctx.sofa_reset()
    for _ in range(6):
        x = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
        got, fresh, exp = ctx.sofa_process_block(x, g), ctx2.sofa_process_block(x, g), ref.process_block(x, g)
        assert (got == fresh).all()
        assert np.abs(got - exp).max() <= _sofa_tol(L, exp)


@pytest.mark.parametrize("C,L,P,B", [(3, 80, 16, 48), (2, 2049, 2048, 2048), (64, 40, 16, 32)])
def test_sofalizer_device_entry_point_equals_host_entry_point(ctx, ctx2, oracle, C, L, P, B):
    """mi355_sofa_process_block_device on buffers from mi355_device_alloc (input and output distinct) against
    mi355_sofa_process_block on a second context fed the same blocks: bit for bit"""
    rng = np.random.default_rng(C + L)
    flt = A.sofa_filters(rng, C, L)
    for c_ in (ctx, ctx2):
        _sofa_pair(c_, oracle, C, L, P, B, flt)
    g = (0.5 + 0.5 * rng.random(C)).astype(np.float32)
    d_in, d_out = ctx.alloc(B * C * 4), ctx.alloc(B * 2 * 4)
    try:
        for blk in range(4):
            x = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
            if blk == 2:
                for c_ in (ctx, ctx2):
                    c_.sofa_set_filter(C - 1, flt[0][1], flt[0][0], 1, 2)
            ctx.h2d(d_in, x)
            ctx.sofa_process_block_device(d_in, d_out, g)
            got = np.zeros((B, 2), np.float32)
            ctx.d2h(got, d_out)
            exp = ctx2.sofa_process_block(x, g)
            assert np.abs(exp).max() > 0 and got.tobytes() == exp.tobytes(), blk
            back = np.zeros((B, C), np.float32)
            ctx.d2h(back, d_in)
            assert back.tobytes() == x.tobytes()                     # the input buffer is read only
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


@pytest.mark.parametrize("C,L,P,B", [(2, 40, 16, 64), (1, 20, 8, 8), (2, 24, 8, 32)])
def test_sofalizer_impulse_reproduces_integer_taps_in_place(ctx, C, L, P, B):
    """taps are distinct small integers (left 1.., right 101.. of channel 0; 201.. / 301.. of channel 1): an impulse at sub-block
    position 0, P - 1, P, B - 1 must bring them back at the right sample of the right ear - a one-sample slip or a swapped ear
    is off by a whole tap"""
    ctx.sofa_setup(C, L, P, B)
    taps = []
    for c in range(C):
        l = np.arange(200 * c + 1, 200 * c + 1 + L, dtype=np.float32)
        r = np.arange(200 * c + 101, 200 * c + 101 + L, dtype=np.float32)
        ctx.sofa_set_filter(c, l, r)
        taps.append((l, r))
    n_tail = -(-L // B) + 1
    for rep, p in enumerate(sorted({0, P - 1, P % B, B - 1})):
        for c in range(C):
            x = np.zeros((B, C), np.float32)
            x[p, c] = 1.0
            g = np.zeros(C, np.float32)
            g[c] = 1.0
            # the other channel runs at gain 1 as well on odd repetitions: its input is silent, its taps must not leak
            if rep % 2:
                g[:] = 1.0
            out = np.concatenate([ctx.sofa_process_block(x if k == 0 else np.zeros_like(x), g) for k in range(n_tail + 1)])
            exp = np.zeros_like(out, dtype=np.float64)
            exp[p:p + L, 0], exp[p:p + L, 1] = taps[c]
            assert (np.round(out) == exp).all(), (p, c)
            assert np.abs(out - exp).max() <= 2e-3, (p, c)


# ------------------------------------------------------------------ hrtfrender

def _sphere(synth, oracle, length):
    data = synth.hrir_sphere_bytes(open(GOLDEN, "rb").read(), length)
    return data, oracle.HrirSphere(data, 44100)


def _hrtf_setup(ctx, data, channels, block, steps, method):
    import mi355fx
    ctx.hrtf_load_sphere(data, 44100)
    ctx.set_flag(mi355fx.FLAG_HRTF_METHOD, method)
    try:
        ctx.hrtf_setup(channels, block, steps)
    finally:
        ctx.set_flag(mi355fx.FLAG_HRTF_METHOD, 0)


@pytest.mark.parametrize("method,length,block,steps,fft", [(1, 100, 500, 2, 1024), (2, 100, 500, 2, 0), (1, 33, 480, 1, 512), (2, 33, 16, 4, 0)])
def test_hrtf_impulse_lands_in_the_right_ear_at_the_right_sample(ctx, oracle, synth, method, length, block, steps, fft):
    """static source well to one side (the synthetic sphere's ears differ in onset and level); impulses in the first and last
    frame of a step: the output is gain x the blended HRIR of each ear, left in [.., 0], right in [.., 1], starting at the
    impulse (the FFT form packs left / right as real / imaginary part of one transform)"""
    data, sphere = _sphere(synth, oracle, length)
    _hrtf_setup(ctx, data, 1, block, steps, method)
    assert ctx.hrtf_transform_size() == fft
    pos, g = np.array([[0.9, 0.1, 0.3]], np.float32), np.array([0.5], np.float32)
    face, uvw = sphere.sample(pos[0])
    left, right = A.hrir_taps(data, face, uvw)
    assert np.abs(left - right).max() > 0.05
    frames = block * steps
    places = [0, block - 1, frames - 1] if steps > 1 else [0, block - 1]
    x = np.zeros((frames, 1), np.float32)
    for k, p in enumerate(places):
        x[p, 0] = 1.0 + k
    n_blocks = 2 + length // frames
    out = np.concatenate([ctx.hrtf_process_block(x if b == 0 else np.zeros_like(x), pos, g).reshape(frames, 2) for b in range(n_blocks)])
    exp = np.zeros((n_blocks * frames, 2))
    for k, p in enumerate(places):
        exp[p:p + length, 0] += 0.5 * (1.0 + k) * left
        exp[p:p + length, 1] += 0.5 * (1.0 + k) * right
    faces, _ = ctx.hrtf_last_lookup()
    assert (faces == face).all()
    assert np.abs(out - exp).max() <= HRTF_TOL_EXACT * max(1.0, np.abs(exp).max())
    assert np.abs(out[:, ::-1] - exp).max() > 1e-2


def _hrtf_static_run(ctx, oracle, synth, length, channels, steps, block, n_blocks, method, seed):
    data, sphere = _sphere(synth, oracle, length)
    _hrtf_setup(ctx, data, channels, block, steps, method)
    ex = oracle.HrtfExact(sphere, channels, steps, block)
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((channels, 3)).astype(np.float32)
    gains = rng.uniform(0.2, 1.0, channels).astype(np.float32)
    worst = scale = 0.0
    for _ in range(n_blocks):
        x = rng.uniform(-1, 1, (steps * block, channels)).astype(np.float32)
        got, e = ctx.hrtf_process_block(x, pos, gains), ex.process_block(x, pos, gains)
        worst, scale = max(worst, float(np.abs(got - e).max())), max(scale, float(np.abs(e).max()))
    return worst, max(1.0, scale)


@pytest.mark.parametrize("length,channels,steps,block,n_blocks,method", [
    (64, 2, 1, 128, 4, 2), (600, 2, 1, 424, 4, 1),      # one interpolation step (FIR; FFT with the window on 1023 points)
    (32, 2, 64, 16, 3, 2), (500, 1, 64, 13, 3, 1),      # 64 steps, the setup limit (the per-step face table has 64 entries)
    (16, 2, 8, 1, 20, 2),                               # block of one frame
    (64, 2, 1, 8, 40, 2), (200, 2, 2, 5, 50, 2),        # blocks shorter than the history: the history row turns over several times
    (520, 1, 1, 8, 150, 1)])                            # the same through the FFT (window 527 -> 1024 points)
def test_hrtf_step_bounds_and_short_blocks_static(ctx, oracle, synth, length, channels, steps, block, n_blocks, method):
    """static sources: the blocks tile one long convolution whatever the block size, so the f64 evaluation is the reference end
    to end"""
    worst, scale = _hrtf_static_run(ctx, oracle, synth, length, channels, steps, block, n_blocks, method, 5 * length + block)
    assert ctx.hrtf_transform_size() == A.hrtf_expected_transform(length, block, method)
    assert worst <= HRTF_TOL_EXACT * scale, (worst, scale)


def test_hrtf_steps_beyond_the_limit_are_refused(ctx, synth, oracle):
    import mi355fx
    data, _ = _sphere(synth, oracle, 8)
    ctx.hrtf_load_sphere(data, 44100)
    for steps in (0, 65):
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.hrtf_setup(1, 16, steps)
        assert e.value.status == mi355fx.ERR_INVALID_ARG
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.hrtf_transform_size()
    assert e.value.status == mi355fx.ERR_NOT_CONFIGURED


@pytest.mark.parametrize("method,length,block,steps,channels", [(1, 400, 300, 4, 3), (2, 90, 77, 4, 3)])
def test_hrtf_device_entry_point_equals_host_entry_point(ctx, ctx2, oracle, synth, method, length, block, steps, channels):
    """mi355_hrtf_process_block_device on buffers from mi355_device_alloc against mi355_hrtf_process_block on a second context
    fed the same blocks and positions: bit for bit"""
    data, _ = _sphere(synth, oracle, length)
    for c_ in (ctx, ctx2):
        _hrtf_setup(c_, data, channels, block, steps, method)
    assert ctx.hrtf_transform_size() == ctx2.hrtf_transform_size() == (1024 if method == 1 else 0)
    frames = block * steps
    rng = np.random.default_rng(length)
    pos = rng.standard_normal((channels, 3)).astype(np.float32)
    d_in, d_out = ctx.alloc(frames * channels * 4), ctx.alloc(frames * 2 * 4)
    try:
        for blk in range(3):
            x = rng.uniform(-1, 1, (frames, channels)).astype(np.float32)
            pos = (pos + 0.5 * rng.standard_normal((channels, 3))).astype(np.float32)
            g = rng.uniform(0.2, 1.0, channels).astype(np.float32)
            ctx.h2d(d_in, x)
            ctx.hrtf_process_block_device(d_in, d_out, pos, g)
            got = np.zeros(frames * 2, np.float32)
            ctx.d2h(got, d_out)
            exp = ctx2.hrtf_process_block(x, pos, g)
            assert np.abs(exp).max() > 0 and got.tobytes() == exp.tobytes(), blk
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
