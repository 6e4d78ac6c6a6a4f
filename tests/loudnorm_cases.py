"""Deterministic audioloudnorm streams and the limiter branches each one claims (labels of tests/loudnorm_restate.py).

Shared by tests/test_loudnorm_cpu.py (restatement == oracle bit for bit, every claim reached, every label covered) and by
tests/test_gpu_loudnorm.py / tests/test_gpu_agroup.py (device against the oracle). Nothing reads a file.

Two kinds of material.

"grid" cases put single samples ON the positions the limiter's bookkeeping distinguishes. They are built so that the gain
is one constant everywhere: the input stays below -70 LUFS (amplitudes of 1e-3, a handful of samples), so above_threshold
is false, env_shortterm is 0 and every delta is 1.0 (imp.rs:383-394, :556-581); gain == gain_next, and the whole gain is
the `offset` setting of +60 dB (10^3 exactly) times the gaussian weights' sum. A sample written as v below arrives in
limiter_buf as v * that constant (~v), so orderings, plateaus and ratios between events are those written here.
Positions are absolute frame numbers; limiter call k covers output frames [k * 19200, (k + 1) * 19200) and in state Out
its detect_peak's n is (position - k * 19200 - 1920).

"programme" cases are a tone with bursts far above the ceiling at default settings, where the gain follows the meters:
the stream-length edges and the misaligned final call."""
import numpy as np

RATE = 192000
F = 19200            # FRAME_SIZE
N0 = 3 * RATE        # GAIN_LOOKAHEAD
LOOK = 1920          # LIMITER_LOOKAHEAD == LIMITER_ATTACK_WINDOW
GRID_KW = dict(offset=60.0)
UNIT = 1e-3          # input value that arrives as ~1.0


class Case:
    """`make` builds the (frames, channels) f64 stream on first use; release() drops it again (the long ones are tens of MB)"""

    def __init__(self, name, channels, make, claims, kw=None, pushes=None, strict_ok=True):
        self.name, self.channels, self._make, self.claims, self.kw = name, channels, make, tuple(claims), dict(kw or {})
        self.pushes = pushes          # list of push sizes in frames (rest is pushed in one piece); None: one push
        self.strict_ok = strict_ok    # False: the reference's frame-wise walk leaves the ring (element-wrap contract only)
        self._x = None

    @property
    def x(self):
        if self._x is None:
            self._x = self._make()
            assert self._x.shape[1] == self.channels
        return self._x

    def release(self):
        self._x = None

    def chunks(self):
        pos = 0
        for n in (self.pushes or []):
            yield self.x[pos:pos + n]
            pos += n
        if pos < len(self.x):
            yield self.x[pos:]

    def __repr__(self):
        return self.name


def _floor(n, ch):
    """background far below the ceiling (arrives as 1e-4), different per channel, no two neighbours equal"""
    t = np.arange(n)
    return np.stack([1e-7 * np.sin(2 * np.pi * (0.0137 + 0.0011 * c) * t + 0.3 * c) for c in range(ch)], 1)


def _grid(events, ch=1, n=N0 + 2 * F + 7):
    return ch, lambda: _grid_now(events, ch, n)


def _grid_now(events, ch, n):
    x = _floor(n, ch)
    for ev in events:
        p, v = ev[0], ev[1]
        c = ev[2] if len(ev) > 2 else 0
        x[p, c] = v * UNIT
    return x


def at(k, n):
    """position that state Out of limiter call k sees at detect_peak's n"""
    return k * F + LOOK + n


def _programme(n, ch, bursts, seed):
    """a 3 kHz tone that carries the loudness (near the target whatever the channel count, so the gain stays within 0.3 .. 1)
    with short 9.6 kHz bursts (start, frames, amplitude) that stay far above the ceiling after the gain"""
    amp = 0.1 / np.sqrt(ch)
    t = np.arange(n) / RATE
    x = np.stack([amp * np.sin(2 * np.pi * (3000.0 + 170 * c) * t) for c in range(ch)], 1)
    for start, length, a in bursts:
        start = start if start >= 0 else n + start
        i = np.arange(length)
        for c in range(ch):
            x[start:start + length, c] = a * (1.0 - 0.07 * c) * np.sin(2 * np.pi * 0.05 * i + 0.9 * c + 0.4)
    return x + 1e-4 * np.random.default_rng(seed).standard_normal(x.shape)


_TAIL = ((-50000, 40, 3.5), (-30000, 30, 5.0), (-21000, 60, 3.0), (-9000, 40, 4.0), (-2500, 30, 5.0), (-400, 50, 3.6))
_BODY = ((1000, 40, 4.0), (200000, 60, 3.5), (203000, 40, 5.0), (420000, 50, 3.0), (560000, 40, 3.8))


def programme(n, ch, seed):
    """the programme material of the length cases for any length: bursts in the body and in the last 50,000 frames"""
    return _programme(n, ch, _BODY + _TAIL, seed)


def _length_case(name, n, ch, claims, pushes=None, strict_ok=True):
    """programme of n frames; one burst ends 300 frames before the last, short limiter call begins, so that call is entered with
    an envelope running and multiplies frames from its first one on"""
    carry = ((-(n % F) - 340, 40, 4.0),) if n % F else ()
    return Case(name, ch, lambda: _programme(n, ch, _BODY + _TAIL + carry, seed=n % 1000 + ch), claims, pushes=pushes, strict_ok=strict_ok)


def cases():
    out = []
    add = lambda name, grid, claims, kw: out.append(Case(name, grid[0], grid[1], claims, kw))

    # ---------------------------------------------------------------- detect_peak: tile edges of the device search
    add("grid_tile_edges",
        _grid([(at(3, 1), 1.2), (at(7, 1023), 1.3), (at(11, 1024), 1.25), (at(15, 1025), 1.35), (at(19, 19199), 1.2)]),
        ["ff.nothing", "out.no_peak", "out.peak_to_attack", "dp.hit_n1", "dp.hit_n1023", "dp.hit_n1024", "dp.hit_n1025", "dp.hit_last",
         "att.ramp_completes_window", "att.to_sustain", "sus.to_release", "rel.ramp_cut_by_call_end", "rel.ramp_completes_to_out",
         "att.ramp_cut_by_call_end", "att.ramp_resumed"], GRID_KW)
    # two candidates in the first tile (the later one higher: an any-hit search that returns it starts the attack 100 frames
    # late and for the wrong value), one more four tiles on
    add("grid_two_in_tile_and_later_tile",
        _grid([(at(3, 500), 1.2), (at(3, 600), 1.6), (at(3, 4700), 1.3), (at(9, 1030), 1.2), (at(9, 2040), 1.7)]),
        ["dp.two_in_tile", "dp.later_tile_candidate", "att.ramp_stopped_at_new_peak", "att.higher_steeper_restart"], GRID_KW)
    # plateau: five equal samples; the first hits through `>=`, each next one through `<=` as a peak of equal height
    add("grid_plateau",
        _grid([(at(3, 2000) + i, 1.3) for i in range(5)] + [(at(8, 1) + i, -1.4) for i in range(3)]),
        ["dp.plateau", "att.lower_peak_env_cnt", "sus.countdown_to_zero", "dp.hit_n1"], GRID_KW)
    # follower veto: a higher sample 11 frames on vetoes (and is the peak itself), one 12 frames on does not
    add("grid_follower_window",
        _grid([(at(3, 2000), 1.2), (at(3, 2011), 1.3), (at(8, 6000), 1.2), (at(8, 6012), 1.25)]),
        ["dp.veto_i11", "dp.no_veto_i12"], GRID_KW)
    # channels: channel 1 peaks while channel 0 is higher but still rising (no maximum there): max_peak comes from channel 0
    add("grid_channels_stereo",
        _grid([(at(3, 3000), 1.2, 1), (at(3, 3000), 1.5, 0), (at(3, 3001), 1.8, 0), (at(9, 500), -1.3, 1)], ch=2),
        ["dp.hit_channel_gt0", "dp.max_from_other_channel"], GRID_KW)
    add("grid_channels_six",
        _grid([(at(3, 3000), 1.2, 4), (at(3, 3000), 1.5, 2), (at(3, 3001), 1.8, 2), (at(9, 1024), -1.3, 5), (at(9, 1024), 1.1, 0)], ch=6),
        ["dp.hit_channel_gt0", "dp.max_from_other_channel", "dp.hit_n1024"], GRID_KW)

    # ---------------------------------------------------------------- attack
    add("grid_attack_second_peak_inside_window",
        _grid([(at(3, 3000), 1.2), (at(3, 3600), 3.0),          # much higher 600 on: restart
               (at(8, 3000), 1.5), (at(8, 4500), 1.55),         # slightly higher 1500 on: extended ramp
               (at(13, 3000), 1.5), (at(13, 3700), 1.2)]),      # lower 700 on: sustain_cnt = env_cnt
        ["att.ramp_stopped_at_new_peak", "att.higher_steeper_restart", "att.higher_shallower_extended", "att.lower_peak_env_cnt",
         "sus.countdown_to_zero", "att.to_sustain"], GRID_KW)
    add("grid_attack_second_peak_after_window",
        _grid([(at(3, 3000), 1.5), (at(3, 8000), 1.2),          # lower: sustain_cnt untouched
               (at(8, 3000), 1.5), (at(8, 8000), 2.0),          # higher, shallower from the finished window
               (at(13, 3000), 1.05), (at(13, 8000), 3.0)]),     # higher, steeper: restart from gain_reduction[1]
        ["att.const_stretch_to_new_peak", "att.lower_peak_window_done", "att.higher_shallower_extended", "att.higher_steeper_restart",
         "att.to_sustain"], GRID_KW)
    # the peak on the first sample of call 6: window and release both complete exactly on a call's last sample
    add("grid_window_ends_on_call_end",
        _grid([(6 * F, 1.5), (12 * F, -1.5)]),
        ["att.window_completes_at_call_end", "att.entered_with_window_done", "rel.ramp_completes_at_call_end", "rel.entered_with_window_done",
         "att.to_sustain", "sus.to_release"], GRID_KW)
    # ramp carried over a call's end with one frame / all but one frame done
    add("grid_attack_ramp_cut",
        _grid([(5 * F + 1, 1.4), (9 * F + 1919, 1.4), (13 * F + 960, -1.4)]),
        ["att.ramp_cut_by_call_end", "att.ramp_resumed", "att.ramp_completes_window"], GRID_KW)

    # ---------------------------------------------------------------- sustain
    add("grid_first_frame_then_higher",
        _grid([(100, 1.5), (LOOK + 3000, 2.0)]),
        ["ff.positive_max", "sus.entered_from_first_frame", "sus.higher_peak_to_attack"], GRID_KW)
    add("grid_first_frame_then_lower",
        _grid([(LOOK, 1.5), (LOOK + 3000, 1.2)]),
        ["ff.positive_max", "sus.entered_from_first_frame", "sus.lower_peak_lookahead", "sus.countdown_to_zero", "sus.to_release"], GRID_KW)
    add("grid_first_frame_alone",
        _grid([(7, 1.5)]),
        ["ff.positive_max", "sus.entered_from_first_frame", "sus.countdown_to_zero", "sus.to_release"], GRID_KW)
    add("grid_first_frame_negative",
        _grid([(100, -1.5), (50, 0.9)]),        # 0.9 is above the ceiling too; nothing limits either, both are clamped
        ["ff.negative_quirk", "clamp.negative", "clamp.positive"], GRID_KW)
    add("grid_first_frame_negative_stereo",
        _grid([(LOOK, -1.5, 1), (3, 0.7, 0)], ch=2),
        ["ff.negative_quirk", "clamp.negative"], GRID_KW)
    # sustain countdown running over a call's end: peak 100 before the end of call 5, a lower one 1000 on
    add("grid_sustain_countdown_cut",
        _grid([(6 * F - 100, 1.5), (6 * F + 900, 1.2)]),
        ["att.lower_peak_env_cnt", "sus.countdown_cut_by_call_end", "sus.countdown_to_zero", "sus.to_release"], GRID_KW)

    # ---------------------------------------------------------------- release: cut by the end of call 3 at env_cnt = 9200, where the
    # current value is g0 - 9200 / 19199 * (1 - g0) = 0.50 for g0 = ceiling / 1.2 (the reference's release ramp runs downwards, sic)
    add("grid_release_then_higher",
        _grid([(3 * F + 10000, 1.2), (4 * F + 6000, 2.0)]),
        ["rel.ramp_cut_by_call_end", "rel.higher_peak_to_attack"], GRID_KW)
    add("grid_release_then_lower",
        _grid([(3 * F + 10000, 1.2), (4 * F + 6000, 1.05)]),
        ["rel.ramp_cut_by_call_end", "rel.lower_peak_to_sustain", "sus.lower_peak_lookahead"], GRID_KW)

    # ---------------------------------------------------------------- stream-length edges (192 kHz frames)
    out.append(Case("len_3s_minus_1", 2, lambda: _programme(N0 - 1, 2, _BODY, 1), ["frame.linear"]))
    out.append(_length_case("len_3s", N0, 2, ["frame.first", "frame.final", "final.no_leftover"]))
    out.append(_length_case("len_3s_plus_1", N0 + 1, 1, ["frame.final", "final.short_call"]))
    out.append(_length_case("len_3s_plus_19199", N0 + 19199, 1, ["frame.final", "final.short_call"]))
    out.append(_length_case("len_3s_plus_19200", N0 + 19200, 2, ["frame.inner", "frame.final", "final.no_leftover"]))
    out.append(_length_case("len_3s_plus_19201", N0 + 19201, 1, ["frame.inner", "final.short_call"]))
    out.append(_length_case("len_single_frame_pushes_across_3s", N0 + 19200 + 3000, 1, ["frame.inner", "final.short_call"],
                            pushes=[N0 - 3] + [1] * 6 + [19190] + [1] * 12))

    # ---------------------------------------------------------------- misaligned final call: (FRAME_SIZE - leftover) % channels != 0
    mis = ["final.short_call", "final.misaligned", "final.misaligned_writes"]
    for ch in (2, 3, 6):
        out.append(_length_case("misaligned_in_bounds_%dch" % ch, 604801, ch, mis))
        out.append(_length_case("misaligned_crossing_%dch" % ch, 610201, ch, mis + ["final.crossing_read", "final.crossing_write", "final.crossing_output"], strict_ok=False))
    out.append(_length_case("misaligned_crossing_931201_2ch", 931201, 2, mis + ["final.crossing_read"], strict_ok=False))
    out.append(_length_case("misaligned_crossing_892801_2ch", 892801, 2, mis + ["final.crossing_read", "final.crossing_write", "final.crossing_output"], strict_ok=False))
    return out


_CACHE = {}


def all_cases():
    if not _CACHE:
        for c in cases():
            _CACHE[c.name] = c
    return list(_CACHE.values())


def names():
    return [c.name for c in all_cases()]


def get(name):
    all_cases()
    return _CACHE[name]
