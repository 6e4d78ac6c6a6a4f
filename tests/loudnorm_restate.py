"""Independent restatement of audioloudnorm's State (audio/audiofx/src/audioloudnorm/imp.rs) with a branch trace.

Written from imp.rs, function by function, NOT from oracle/loudnorm_oracle.c or csrc/loudnorm.hip: it is the second reading
of the reference that the C oracle (and through it both device transcriptions of the limiter) is checked against,
BIT FOR BIT (tests/test_loudnorm_cpu.py). Arithmetic is scalar Python `float` (IEEE binary64, never fused) in the
reference's expression order with math.pow / math.exp, i.e. the libm the oracle links. The two loudness meters are
oracle.EbuR128 instances (I | S | LRA | sample peak): the meters are not under test here.

`fast=True` (the default) replaces three loops by numpy: the per-sample fills (one multiply chain per element, the same
expression element-wise), the output copy, and detect_peak's search. The literal serial loops stay (`fast=False`) and
the two are compared in tests/test_loudnorm_cpu.py, detect_peak on random rings with plateaus. The limiter's state
machine and every envelope are scalar in both modes.

Ring contract. The reference takes a frame as limiter_buf[index..index + channels] (unchecked) and wraps `index` once
per frame. process_final_frame advances limiter_buf_index by FRAME_SIZE - next_frame_size, frames instead of
frames * channels (imp.rs:766-771), so the last, short limiter call of a stream can start at an index that is no
multiple of `channels`; a frame that then starts less than `channels` elements before the ring's end lies partly
outside the allocation. That is undefined in the reference. With element_wrap=False this restatement raises
RingOverrun there instead of guessing; with element_wrap=True it takes the project's stated contract:
element c of the frame at `index` is limiter_buf[(index + c) % len], which is the reference's walk wherever that
walk is in bounds.

Trace. Every branch of the limiter, of the first-frame scan, of the output clamp and the situations of detect_peak's
search that matter to the device's tiled search are recorded as labels (LABELS below) in State.trace (a set) and, with
the limiter call they occurred in, in State.events. State.calls is the index trace: one record per true_peak_limiter
call."""
import math

import numpy as np

GAIN_LOOKAHEAD = 3 * 192000
FRAME_SIZE = 19200
LIMITER_ATTACK_WINDOW = 1920
LIMITER_RELEASE_WINDOW = 19200
LIMITER_LOOKAHEAD = 1920
TILE = 1024   # the device searches n = 1 + TILE * k + lane; only the trace knows about it

FIRST, INNER, FINAL, LINEAR = "First", "Inner", "Final", "Linear"
OUT, ATTACK, SUSTAIN, RELEASE = "Out", "Attack", "Sustain", "Release"

LABELS = {
    # Out (true_peak_limiter_out)
    "out.peak_to_attack": "Out: peak found, attack starts LIMITER_ATTACK_WINDOW before it",
    "out.no_peak": "Out: nothing found, the call passes through",
    # Attack (true_peak_limiter_attack)
    "att.ramp_completes_window": "ramp ran and env_cnt reached the window",
    "att.ramp_cut_by_call_end": "ramp cut by the call's end, env_cnt carried",
    "att.ramp_resumed": "a later call continues a ramp with the carried env_cnt",
    "att.ramp_stopped_at_new_peak": "ramp stopped because smp_cnt == new_peak_smp_cnt",
    "att.const_stretch_to_new_peak": "window finished, constant gain_reduction[1] up to the new peak's attack point",
    "att.higher_steeper_restart": "higher peak, new_slope <= old_slope: attack restarts from the current value",
    "att.higher_shallower_extended": "higher peak, shallower slope: ramp extended past the old peak, new_end > 1.0",
    "att.higher_shallower_clamped": "the same with new_end clamped up to 1.0 (EXEMPT, see UNREACHABLE)",
    "att.lower_peak_env_cnt": "lower or equal peak with env_cnt < window: sustain_cnt = env_cnt",
    "att.lower_peak_window_done": "lower or equal peak with the window finished: sustain_cnt untouched",
    "att.to_sustain": "window finished before the call's end: Sustain",
    "att.window_completes_at_call_end": "window finished exactly on the call's last sample: still Attack in the next call",
    "att.entered_with_window_done": "call entered in Attack with env_cnt == window (the follow-up of the label above)",
    # Sustain (true_peak_limiter_sustain)
    "sus.higher_peak_to_attack": "higher peak: Attack from gain_reduction[1]",
    "sus.lower_peak_lookahead": "lower or equal peak: sustain_cnt = LIMITER_LOOKAHEAD",
    "sus.countdown_to_zero": "pending sustain_cnt counted down to zero: None",
    "sus.countdown_cut_by_call_end": "pending sustain_cnt cut by the call's end, remainder carried",
    "sus.to_release": "no peak, nothing pending: Release",
    "sus.entered_from_first_frame": "Sustain entered by the first-frame scan",
    # Release (true_peak_limiter_release)
    "rel.higher_peak_to_attack": "peak needing more reduction than the current value: constant stretch * gain_reduction[1], Attack",
    "rel.lower_peak_to_sustain": "peak needing no more than the current value: Sustain at the current value",
    "rel.ramp_cut_by_call_end": "release ramp cut by the call's end, env_cnt carried",
    "rel.ramp_completes_to_out": "release ramp completes inside the call: Out",
    "rel.ramp_completes_at_call_end": "release ramp completes exactly on the call's last sample: still Release in the next call",
    "rel.entered_with_window_done": "call entered in Release with env_cnt == window: Out at once",
    # first frame (true_peak_limiter_first_frame)
    "ff.positive_max": "signed max positive and above the ceiling: Sustain with gain_reduction[1] = target_tp / max",
    "ff.negative_quirk": "largest magnitude above the ceiling but negative: the signed `max` fails the test, only the clamp acts",
    "ff.nothing": "nothing above the ceiling in the first LIMITER_LOOKAHEAD + 1 frames",
    # output copy
    "clamp.positive": "a positive sample above the ceiling clamped",
    "clamp.negative": "a negative sample below -ceiling clamped",
    # detect_peak
    "dp.hit_n1": "hit at n = 1 (first candidate of the first tile)",
    "dp.hit_last": "hit at n = samples - 1",
    "dp.hit_n1023": "hit at n = 1023",
    "dp.hit_n1024": "hit at n = 1024 (last lane of the first tile)",
    "dp.hit_n1025": "hit at n = 1025 (first lane of the second tile)",
    "dp.two_in_tile": "a second candidate in the hit's 1024-tile: the earlier wins",
    "dp.later_tile_candidate": "a candidate in a later tile than the hit's",
    "dp.plateau": "hit on a plateau: predecessor or successor equal to the sample (<= / >=)",
    "dp.veto_i11": "three-point maximum vetoed by a higher follower at i = 11 only",
    "dp.no_veto_i12": "hit although the sample at i = 12 is higher",
    "dp.hit_channel_gt0": "hit on a channel c > 0 while channel 0 does not hit",
    "dp.max_from_other_channel": "max_peak taken from a channel that did not hit",
    # frames and the misaligned final call
    "frame.first": "process_first_frame", "frame.inner": "process_inner_frame", "frame.final": "process_final_frame",
    "frame.linear": "process_first_frame_is_last + process_linear_frame",
    "final.no_leftover": "drain with nothing left over: 29 whole limiter calls, no short one",
    "final.short_call": "the last limiter call is short",
    "final.misaligned": "the short call starts at an index that is no multiple of `channels`",
    "final.misaligned_writes": "an envelope multiplies frames in the misaligned call",
    "final.crossing_read": "a frame read in the misaligned call straddles the ring's end (element_wrap only)",
    "final.crossing_write": "a frame multiplied in the misaligned call straddles the ring's end (element_wrap only)",
    "final.crossing_output": "a frame of the output copy straddles the ring's end (element_wrap only)",
}

# Labels no input can reach, each with the argument from imp.rs. Nothing of Out, Sustain, Release or the first frame.
UNREACHABLE = {
    "att.higher_shallower_clamped":
        "new_end = (gain_reduction - g0) / old_slope = (g0 - gain_reduction) / (g0 - g1) (imp.rs:1025-1026), reached only under "
        "gain_reduction < g1 (:981), with g0 = gain_reduction[0], g1 = gain_reduction[1]. g0 > g1 holds whenever the state is "
        "Attack, by induction over the five places that set the pair on the way into Attack: Out sets (1.0, tp / peak) with "
        "peak > tp (:859-860, :1477); Sustain sets (g1, r) under r < g1 (:1157-1162); Release sets (current, r) under "
        "r < current (:1242, :1269-1270); the restart sets (current, r) under r < g1 and new_slope <= old_slope, i.e. "
        "current - r >= g0 - g1 > 0 (:991-1001); the extension itself sets (g0 + new_start * old_slope, r), and with "
        "new_end > 1 exact arithmetic gives r + (g0 - g1) there, which exceeds r by the old, positive difference (:1039-1043). "
        "IEEE subtraction is monotone, so gain_reduction < g1 gives fl(g0 - gain_reduction) >= fl(g0 - g1) > 0, and the "
        "correctly rounded quotient of a >= b > 0 is >= 1.0. So new_end < 1.0 never holds and f64::max(new_end, 1.0) never "
        "changes its argument. tests/test_loudnorm_cpu.py asserts g0 > g1 > gain_reduction at every entry to the branch in "
        "every case and checks the quotient on adjacent doubles.",
}


class RingOverrun(IndexError):
    """the reference's frame-wise walk would leave limiter_buf (undefined behaviour there)"""


class State:
    def __init__(self, oracle, channels, loudness_target=-24.0, loudness_range_target=7.0, max_true_peak=-2.0, offset=0.0,
                 element_wrap=False, fast=True):
        mode = oracle.EB_I | oracle.EB_S | oracle.EB_LRA | oracle.EB_SAMPLE_PEAK
        self.r128_in = oracle.EbuR128(channels, 192000, mode)
        self.r128_out = oracle.EbuR128(channels, 192000, mode)
        self.channels = channels
        self.element_wrap, self.fast = element_wrap, fast
        self.buf = np.zeros(GAIN_LOOKAHEAD * channels)
        self.limiter_buf = np.zeros((2 * FRAME_SIZE + LIMITER_LOOKAHEAD) * channels)
        self.prev_smp = [0.0] * channels
        self.current_samples_per_frame = GAIN_LOOKAHEAD
        self.buf_index = 0
        self.prev_buf_index = 0
        self.limiter_buf_index = 0
        self.index = 1
        self.limiter_state = OUT
        self.offset = math.pow(10.0, offset / 20.0)
        self.target_tp = math.pow(10.0, max_true_peak / 20.0)
        self.target_i = loudness_target
        self.target_lra = loudness_range_target
        self.delta = [0.0] * 30
        self.weights = init_gaussian_filter()
        self.prev_delta = 0.0
        self.gain_reduction = [0.0, 0.0]
        self.env_cnt = 0
        self.sustain_cnt = None
        self.frame_type = FIRST
        self.above_threshold = False
        # adapter
        self.adapter = np.zeros(0)
        # trace
        self.trace = set()
        self.events = []      # (limiter call number, label)
        self.calls = []       # dict per true_peak_limiter call
        self.shallow_entries = []   # (g0, g1, gain_reduction) at every entry to the shallower-slope branch
        self._from_first_frame = False
        self._misaligned_call = False

    # ------------------------------------------------------------------ trace
    def _t(self, label):
        assert label in LABELS, label
        self.trace.add(label)
        self.events.append((len(self.calls) - 1, label))

    # ------------------------------------------------------------------ adapter (drain_full_frames / drain)
    def push(self, data):
        a = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
        self.adapter = np.concatenate([self.adapter, a])
        outs = []
        while self.adapter.size >= self.channels * self.current_samples_per_frame:
            take = self.channels * self.current_samples_per_frame
            src, self.adapter = self.adapter[:take], self.adapter[take:]
            outs.append(self.process(src))
        return np.concatenate(outs) if outs else np.zeros(0)

    def drain(self):
        src, self.adapter = self.adapter, np.zeros(0)
        if self.current_samples_per_frame == FRAME_SIZE:
            self.frame_type = FINAL
        elif src.size == 0:
            return None   # FlowError::Eos
        return self.process(src)

    # ------------------------------------------------------------------ frames
    def process(self, src):
        self.r128_in.add_frames(src)
        if self.frame_type == FIRST and src.size // self.channels < self.current_samples_per_frame:
            self.process_first_frame_is_last()
        if self.frame_type == FIRST:
            return self.process_first_frame(src)
        if self.frame_type == INNER:
            return self.process_inner_frame(src)
        if self.frame_type == FINAL:
            return self.process_final_frame(src)
        return self.process_linear_frame(src)

    def process_first_frame_is_last(self):
        global_ = self.r128_in.loudness_global()
        true_peak = 0.0
        for c in range(self.channels):
            peak = self.r128_in.sample_peak(c)
            if c == 0 or peak > true_peak:
                true_peak = peak
        offset = math.pow(10.0, (self.target_i - global_) / 20.0)
        offset_tp = true_peak * offset
        self.offset = offset if offset_tp < self.target_tp else self.target_tp / true_peak
        self.frame_type = LINEAR

    def process_first_frame(self, src):
        self.trace.add("frame.first")
        self.buf[:] = src
        shortterm = self.r128_in.loudness_shortterm()
        if shortterm < -70.0:
            self.above_threshold = False
            env_shortterm = 0.0
        else:
            self.above_threshold = True
            env_shortterm = self.target_i - shortterm
        for i in range(30):
            self.delta[i] = math.pow(10.0, env_shortterm / 20.0)
        self.prev_delta = self.delta[self.index]
        n = self.limiter_buf.size
        if self.fast:
            self.limiter_buf[:] = self.buf[:n] * self.prev_delta * self.offset
        else:
            for i in range(n):
                self.limiter_buf[i] = float(self.buf[i]) * self.prev_delta * self.offset
        self.buf_index = n
        self.limiter_buf_index = 0
        dst = self.true_peak_limiter(FRAME_SIZE)
        self.r128_out.add_frames(dst)
        self.current_samples_per_frame = FRAME_SIZE
        self.frame_type = INNER
        return dst

    def _gains(self):
        gain = self.gaussian_filter(self.index + 10 if self.index + 10 < 30 else self.index + 10 - 30)
        gain_next = self.gaussian_filter(self.index + 11 if self.index + 11 < 30 else self.index + 11 - 30)
        return gain, gain_next

    def _fill_check(self):
        # the fills take limiter_buf[limiter_buf_index..+channels] as a slice too; they only ever run before the sic advance
        if self.limiter_buf_index % self.channels and not self.element_wrap:
            raise RingOverrun("fill at misaligned limiter_buf_index %d" % self.limiter_buf_index)

    def process_fill_inner_frame(self, src):
        gain, gain_next = self._gains()
        ch = self.channels
        frames = src.size // ch
        assert frames <= FRAME_SIZE
        self._fill_check()
        blen, llen = self.buf.size, self.limiter_buf.size
        if self.fast:
            e = np.arange(frames * ch)
            n = (e // ch).astype(np.float64)
            current_gain = (gain + ((n / float(FRAME_SIZE)) * (gain_next - gain))) * self.offset
            read = self.buf[(self.buf_index + e) % blen]          # buf_read and buf_write never overlap (210 ms apart)
            self.buf[(self.prev_buf_index + e) % blen] = src[:frames * ch]
            self.limiter_buf[(self.limiter_buf_index + e) % llen] = read * current_gain
            self.limiter_buf_index = (self.limiter_buf_index + frames * ch) % llen
            self.prev_buf_index = (self.prev_buf_index + frames * ch) % blen
            self.buf_index = (self.buf_index + frames * ch) % blen
            return
        for n in range(frames):
            for c in range(ch):
                self.buf[self.prev_buf_index + c] = src[n * ch + c]
            current_gain = (gain + ((float(n) / float(FRAME_SIZE)) * (gain_next - gain))) * self.offset
            for c in range(ch):
                self.limiter_buf[(self.limiter_buf_index + c) % llen] = float(self.buf[self.buf_index + c]) * current_gain
            self.limiter_buf_index += ch
            if self.limiter_buf_index >= llen:
                self.limiter_buf_index -= llen
            self.prev_buf_index += ch
            if self.prev_buf_index >= blen:
                self.prev_buf_index -= blen
            self.buf_index += ch
            if self.buf_index >= blen:
                self.buf_index -= blen

    def process_update_gain_inner_frame(self):
        global_ = self.r128_in.loudness_global()
        shortterm = self.r128_in.loudness_shortterm()
        relative_threshold = self.r128_in.relative_threshold()
        if not self.above_threshold:
            if shortterm > -70.0:
                self.prev_delta *= 1.0058
            shortterm_out = self.r128_out.loudness_shortterm()
            if shortterm_out >= self.target_i:
                self.above_threshold = True
        if shortterm < relative_threshold or shortterm <= -70.0 or not self.above_threshold:
            self.delta[self.index] = self.prev_delta
        else:
            if abs(shortterm - global_) < (self.target_lra / 2.0):
                env_global = shortterm - global_
            elif (self.target_lra / 2.0) * (shortterm - global_) < 0.0:
                env_global = -1.0
            else:
                env_global = 1.0
            env_shortterm = self.target_i - shortterm
            self.delta[self.index] = math.pow(10.0, (env_global + env_shortterm) / 20.0)
        self.prev_delta = self.delta[self.index]
        self.index += 1
        if self.index >= 30:
            self.index -= 30

    def process_inner_frame(self, src):
        self.trace.add("frame.inner")
        self.process_fill_inner_frame(src)
        dst = self.true_peak_limiter(self.current_samples_per_frame)
        self.r128_out.add_frames(dst)
        self.process_update_gain_inner_frame()
        return dst

    def process_fill_final_frame(self, idx, num_samples):
        ch = self.channels
        gain, gain_next = self._gains()
        if num_samples > idx:
            self._fill_check()
        blen, llen = self.buf.size, self.limiter_buf.size
        if self.fast:
            count = max(0, num_samples - idx)
            e = np.arange(count * ch)
            n = (idx + e // ch).astype(np.float64)
            current_gain = (gain + ((n / float(num_samples)) * (gain_next - gain))) * self.offset
            self.limiter_buf[(self.limiter_buf_index + e) % llen] = self.buf[(self.buf_index + e) % blen] * current_gain
            self.limiter_buf_index = (self.limiter_buf_index + count * ch) % llen
            self.buf_index = (self.buf_index + count * ch) % blen
            return
        for n in range(idx, num_samples):
            current_gain = (gain + ((float(n) / float(num_samples)) * (gain_next - gain))) * self.offset
            for c in range(ch):
                self.limiter_buf[(self.limiter_buf_index + c) % llen] = float(self.buf[self.buf_index + c]) * current_gain
            self.limiter_buf_index += ch
            if self.limiter_buf_index >= llen:
                self.limiter_buf_index -= llen
            self.buf_index += ch
            if self.buf_index >= blen:
                self.buf_index -= blen

    def process_final_frame(self, src):
        self.trace.add("frame.final")
        ch = self.channels
        num_samples = src.size // ch
        self.process_fill_inner_frame(src)
        if num_samples != FRAME_SIZE:
            self.process_fill_final_frame(num_samples, FRAME_SIZE)
        out_num_samples = 30 * FRAME_SIZE - (FRAME_SIZE - num_samples)
        if num_samples == 0:
            self.trace.add("final.no_leftover")
        dst = np.zeros(out_num_samples * ch)
        smp_cnt = 0
        while smp_cnt < out_num_samples:
            frame_size = min(out_num_samples - smp_cnt, FRAME_SIZE)
            part = self.true_peak_limiter(frame_size)
            dst[smp_cnt * ch:(smp_cnt + frame_size) * ch] = part
            smp_cnt += frame_size
            if smp_cnt == out_num_samples:
                break
            self.r128_out.add_frames(part)
            self.process_update_gain_inner_frame()
            next_frame_size = min(out_num_samples - smp_cnt, FRAME_SIZE)
            self.process_fill_final_frame(0, next_frame_size)
            if next_frame_size < FRAME_SIZE:
                self.limiter_buf_index += FRAME_SIZE - next_frame_size   # frames, not frames * channels (imp.rs:766-771)
                if self.limiter_buf_index >= self.limiter_buf.size:
                    self.limiter_buf_index -= self.limiter_buf.size
        return dst

    def process_linear_frame(self, src):
        self.trace.add("frame.linear")
        if self.fast:
            dst = src * self.offset
        else:
            dst = np.array([float(v) * self.offset for v in src])
        self.r128_out.add_frames(dst)
        return dst

    # ------------------------------------------------------------------ ring access
    def _frame(self, index, what):
        """element indices of the frame limiter_buf[index..index + channels]"""
        ch, llen = self.channels, self.limiter_buf.size
        if index + ch <= llen:
            return range(index, index + ch)
        if not self.element_wrap:
            raise RingOverrun("%s: frame at %d of a ring of %d, %d channels" % (what, index, llen, ch))
        self._t("final.crossing_" + what)
        return [(index + c) % llen for c in range(ch)]

    def _mul_frame(self, index, g):
        lb = self.limiter_buf
        for i in self._frame(index, "write"):
            lb[i] = float(lb[i]) * g
        index += self.channels
        if index >= lb.size:
            index -= lb.size
        return index

    def _start(self, smp_cnt):
        index = self.limiter_buf_index + smp_cnt * self.channels
        if index >= self.limiter_buf.size:
            index -= self.limiter_buf.size
        return index

    def _wrote(self, count):
        if count and self._misaligned_call:
            self._t("final.misaligned_writes")

    # ------------------------------------------------------------------ limiter
    def true_peak_limiter_out(self, smp_cnt, nb_samples):
        peak = self.detect_peak(smp_cnt, nb_samples - smp_cnt)
        if peak is not None:
            peak_delta, peak_value = peak
            self._t("out.peak_to_attack")
            self.limiter_state = ATTACK
            self.env_cnt = 0
            self.sustain_cnt = None
            self.gain_reduction[0] = 1.0
            self.gain_reduction[1] = self.target_tp / peak_value
            smp_cnt += LIMITER_LOOKAHEAD + peak_delta - LIMITER_ATTACK_WINDOW
        else:
            self._t("out.no_peak")
            smp_cnt = nb_samples
        return smp_cnt

    def true_peak_limiter_attack(self, smp_cnt, nb_samples):
        gr = self.gain_reduction
        W = float(LIMITER_ATTACK_WINDOW) - 1.0
        peak = self.detect_peak(smp_cnt, nb_samples - smp_cnt)
        new_peak_smp_cnt = None
        if peak is not None:
            new_peak_smp_cnt = smp_cnt + peak[0]
        if smp_cnt == 0 and self.env_cnt == LIMITER_ATTACK_WINDOW:
            self._t("att.entered_with_window_done")
        elif smp_cnt == 0 and self.env_cnt > 0:
            self._t("att.ramp_resumed")
        index = self._start(smp_cnt)
        ramped, stopped = 0, False
        while self.env_cnt < LIMITER_ATTACK_WINDOW and smp_cnt < nb_samples:
            if new_peak_smp_cnt is not None and smp_cnt == new_peak_smp_cnt:
                stopped = True
                break
            env = gr[0] - (self.env_cnt / W * (gr[0] - gr[1]))
            index = self._mul_frame(index, env)
            smp_cnt += 1
            self.env_cnt += 1
            ramped += 1
        self._wrote(ramped)
        if stopped:
            self._t("att.ramp_stopped_at_new_peak")
        elif ramped and self.env_cnt == LIMITER_ATTACK_WINDOW:
            self._t("att.ramp_completes_window")
        elif ramped:
            self._t("att.ramp_cut_by_call_end")

        if new_peak_smp_cnt is not None:
            assert smp_cnt < nb_samples
            if smp_cnt < new_peak_smp_cnt:
                self._t("att.const_stretch_to_new_peak")
                for _ in range(smp_cnt, new_peak_smp_cnt):
                    index = self._mul_frame(index, gr[1])
                self._wrote(new_peak_smp_cnt - smp_cnt)
                smp_cnt = new_peak_smp_cnt
            assert smp_cnt < nb_samples
            peak_value = peak[1]
            gain_reduction = self.target_tp / peak_value
            if gain_reduction < gr[1]:
                current_gain_reduction = gr[0] - (self.env_cnt / W * (gr[0] - gr[1]))
                old_slope = -(gr[0] - gr[1])
                new_slope = -(current_gain_reduction - gain_reduction)
                if new_slope <= old_slope:
                    self._t("att.higher_steeper_restart")
                    self.limiter_state = ATTACK
                    gr[0] = current_gain_reduction
                    gr[1] = gain_reduction
                    self.env_cnt = 0
                    self.sustain_cnt = None
                else:
                    self.shallow_entries.append((gr[0], gr[1], gain_reduction))
                    new_end = (gain_reduction - gr[0]) / old_slope
                    if new_end != new_end or new_end < 1.0:    # f64::max(new_end, 1.0): the non-NaN / larger one
                        self._t("att.higher_shallower_clamped")
                        new_end = 1.0
                    else:
                        self._t("att.higher_shallower_extended")
                    new_start = new_end - 1.0
                    gr[0] = gr[0] + new_start * old_slope
                    gr[1] = gain_reduction
                    cur_pos = (current_gain_reduction - gr[0]) / old_slope
                    if cur_pos < 0.0:          # f64::clamp: NaN stays NaN
                        cur_pos = 0.0
                    elif cur_pos > 1.0:
                        cur_pos = 1.0
                    pos = W * cur_pos
                    self.env_cnt = 0 if pos != pos else int(pos)    # `as usize`: truncates, NaN -> 0 (pos is in [0, 1919])
                    self.sustain_cnt = self.env_cnt
                return smp_cnt
            if self.env_cnt < LIMITER_ATTACK_WINDOW:
                self._t("att.lower_peak_env_cnt")
                self.sustain_cnt = self.env_cnt
            else:
                self._t("att.lower_peak_window_done")

        if self.env_cnt == LIMITER_ATTACK_WINDOW and smp_cnt < nb_samples:
            self._t("att.to_sustain")
            self.limiter_state = SUSTAIN
        elif self.env_cnt == LIMITER_ATTACK_WINDOW:
            self._t("att.window_completes_at_call_end")
        return smp_cnt

    def true_peak_limiter_sustain(self, smp_cnt, nb_samples):
        gr = self.gain_reduction
        if self._from_first_frame:
            self._t("sus.entered_from_first_frame")
            self._from_first_frame = False
        peak = self.detect_peak(smp_cnt, nb_samples - smp_cnt)
        sustain_cnt = peak[0] if peak is not None else self.sustain_cnt
        if sustain_cnt is not None:
            index = self._start(smp_cnt)
            s = 0
            while s < sustain_cnt and smp_cnt < nb_samples:
                index = self._mul_frame(index, gr[1])
                smp_cnt += 1
                s += 1
            self._wrote(s)
            if peak is not None:
                gain_reduction = self.target_tp / peak[1]
                if gain_reduction < gr[1]:
                    self._t("sus.higher_peak_to_attack")
                    self.limiter_state = ATTACK
                    self.env_cnt = 0
                    self.sustain_cnt = None
                    gr[0] = gr[1]
                    gr[1] = gain_reduction
                else:
                    self._t("sus.lower_peak_lookahead")
                    self.sustain_cnt = LIMITER_LOOKAHEAD
            else:
                self.sustain_cnt -= s
                if self.sustain_cnt == 0:
                    self._t("sus.countdown_to_zero")
                    self.sustain_cnt = None
                else:
                    assert smp_cnt == nb_samples
                    self._t("sus.countdown_cut_by_call_end")
        else:
            self._t("sus.to_release")
            self.limiter_state = RELEASE
            gr[0] = gr[1]
            gr[1] = 1.0
            self.env_cnt = 0
        return smp_cnt

    def true_peak_limiter_release(self, smp_cnt, nb_samples):
        gr = self.gain_reduction
        W = float(LIMITER_RELEASE_WINDOW) - 1.0
        index = self._start(smp_cnt)
        peak = self.detect_peak(smp_cnt, nb_samples - smp_cnt)
        if peak is not None:
            peak_delta, peak_value = peak
            gain_reduction = self.target_tp / peak_value
            current_gain_reduction = gr[0] - (self.env_cnt / W * (gr[1] - gr[0]))
            if gain_reduction < current_gain_reduction:
                self._t("rel.higher_peak_to_attack")
                assert smp_cnt + peak_delta < nb_samples
                for _ in range(peak_delta):
                    index = self._mul_frame(index, gr[1])
                    smp_cnt += 1
                    assert smp_cnt < nb_samples
                self._wrote(peak_delta)
                self.limiter_state = ATTACK
                self.env_cnt = 0
                self.sustain_cnt = None
                gr[0] = current_gain_reduction
                gr[1] = gain_reduction
            else:
                self._t("rel.lower_peak_to_sustain")
                gr[1] = current_gain_reduction
                self.limiter_state = SUSTAIN
            return smp_cnt
        if smp_cnt == 0 and self.env_cnt == LIMITER_RELEASE_WINDOW:
            self._t("rel.entered_with_window_done")
        ramped = 0
        while self.env_cnt < LIMITER_RELEASE_WINDOW and smp_cnt < nb_samples:
            env = gr[0] - (self.env_cnt / W * (gr[1] - gr[0]))
            index = self._mul_frame(index, env)
            smp_cnt += 1
            self.env_cnt += 1
            ramped += 1
        self._wrote(ramped)
        if smp_cnt < nb_samples:
            if ramped:
                self._t("rel.ramp_completes_to_out")
            self.limiter_state = OUT
        elif ramped and self.env_cnt == LIMITER_RELEASE_WINDOW:
            self._t("rel.ramp_completes_at_call_end")
        elif ramped:
            self._t("rel.ramp_cut_by_call_end")
        return smp_cnt

    def true_peak_limiter_first_frame(self):
        ch = self.channels
        assert self.limiter_buf_index == 0
        max_ = 0.0
        largest = 0.0
        for i in range((LIMITER_LOOKAHEAD + 1) * ch):
            sample = float(self.limiter_buf[i])
            if abs(sample) > max_:
                max_ = sample          # the signed sample is kept (imp.rs:1342-1343)
            largest = max(largest, abs(sample))
        for c in range(ch):
            self.prev_smp[c] = abs(float(self.limiter_buf[LIMITER_LOOKAHEAD * ch + c]))
        if max_ > self.target_tp:
            self._t("ff.positive_max")
            self.limiter_state = SUSTAIN
            self.sustain_cnt = LIMITER_LOOKAHEAD
            self.gain_reduction[1] = self.target_tp / max_
            self._from_first_frame = True
        elif largest > self.target_tp:
            self._t("ff.negative_quirk")
        else:
            self._t("ff.nothing")

    def true_peak_limiter(self, nb_samples):
        ch, llen = self.channels, self.limiter_buf.size
        short = self.frame_type == FINAL and nb_samples < FRAME_SIZE
        self._misaligned_call = self.limiter_buf_index % ch != 0
        self.calls.append({"call": len(self.calls), "frame_type": self.frame_type, "nb": nb_samples, "index": self.limiter_buf_index,
                           "misaligned_by": self.limiter_buf_index % ch, "state_in": self.limiter_state})
        if short:
            self._t("final.short_call")
        if self._misaligned_call:
            self._t("final.misaligned")
        if self.frame_type == FIRST:
            self.true_peak_limiter_first_frame()
        smp_cnt = 0
        while smp_cnt < nb_samples:
            if self.limiter_state == OUT:
                smp_cnt = self.true_peak_limiter_out(smp_cnt, nb_samples)
            elif self.limiter_state == ATTACK:
                smp_cnt = self.true_peak_limiter_attack(smp_cnt, nb_samples)
            elif self.limiter_state == SUSTAIN:
                smp_cnt = self.true_peak_limiter_sustain(smp_cnt, nb_samples)
            else:
                smp_cnt = self.true_peak_limiter_release(smp_cnt, nb_samples)
        tp = self.target_tp
        if self.fast:
            if self._walk_crosses(self.limiter_buf_index, nb_samples):
                if not self.element_wrap:
                    raise RingOverrun("output copy: walk from %d over %d frames" % (self.limiter_buf_index, nb_samples))
                self._t("final.crossing_output")
            dst = self.limiter_buf[(self.limiter_buf_index + np.arange(nb_samples * ch)) % llen]
            hi, lo = dst > tp, dst < -tp       # o.abs() > tp, then tp * signum(o)
            dst[hi] = tp * 1.0
            dst[lo] = tp * -1.0
            if hi.any():
                self._t("clamp.positive")
            if lo.any():
                self._t("clamp.negative")
        else:
            dst = np.zeros(nb_samples * ch)
            index = self.limiter_buf_index
            for n in range(nb_samples):
                for c, i in enumerate(self._frame(index, "output")):
                    o = float(self.limiter_buf[i])
                    if abs(o) > tp:
                        self._t("clamp.negative" if math.copysign(1.0, o) < 0 else "clamp.positive")
                        o = tp * math.copysign(1.0, o)
                    dst[n * ch + c] = o
                index += ch
                if index >= llen:
                    index -= llen
        self.calls[-1]["state_out"] = self.limiter_state
        self.calls[-1]["labels"] = sorted({l for k, l in self.events if k == len(self.calls) - 1})
        self._misaligned_call = False
        return dst

    def _walk_crosses(self, start, nframes):
        """does a frame-wise walk of `nframes` frames from element `start` meet a frame that straddles the ring's end?"""
        return start % self.channels != 0 and start + nframes * self.channels > self.limiter_buf.size

    # ------------------------------------------------------------------ detect_peak
    def detect_peak(self, offset, samples):
        ch, llen = self.channels, self.limiter_buf.size
        index = self.limiter_buf_index + (offset + LIMITER_LOOKAHEAD) * ch
        if index >= llen:
            index -= llen
        if self.fast:
            res = self._detect_fast(index, samples)
        else:
            res = detect_peak_serial(self.limiter_buf, ch, index, samples, self.target_tp, self.prev_smp,
                                     lambda i, what="read": self._frame(i, what))
        self._detect_labels(index, samples, res)
        return res

    def _window(self, index, frames):
        """|limiter_buf| of `frames` frames from element `index`, every element wrapped on its own: (frames, ch)"""
        ch, llen = self.channels, self.limiter_buf.size
        return np.abs(self.limiter_buf[(index + np.arange(frames * ch)) % llen]).reshape(frames, ch)

    def _detect_fast(self, index, samples):
        if samples == 0:
            return None
        A = self._window(index, samples + 12)
        hit = detect_candidates(A, samples, self.target_tp)
        rows = np.flatnonzero(hit.any(axis=1))
        n = int(rows[0]) if rows.size else None
        walked = samples if n is None else n + 1        # frames n = 0 .. walked-1 were taken as `this`, each with its `next`
        if self._walk_crosses(index, walked + 1):
            if not self.element_wrap:
                raise RingOverrun("detect_peak: walk from %d over %d frames" % (index, walked + 1))
            self._t("final.crossing_read")
        if n is None:
            self.prev_smp = [float(v) for v in A[samples - 1]]
            return None
        self.prev_smp = [float(v) for v in A[n]]
        return n, float(A[n].max())

    def _detect_labels(self, index, samples, res):
        if res is None or samples < 2:
            if samples >= 2:
                self._veto_labels(self._window(index, samples + 13), samples, samples)
            return
        n = res[0]
        A = self._window(index, samples + 13)
        cand = detect_candidates(A, samples, self.target_tp)
        any_c = cand.any(axis=1)
        if n == 1:
            self._t("dp.hit_n1")
        if n == samples - 1:
            self._t("dp.hit_last")
        if n in (1023, 1024, 1025):
            self._t("dp.hit_n%d" % n)
        tile = (n - 1) // TILE
        later = np.flatnonzero(any_c[n + 1:]) + n + 1
        if (((later - 1) // TILE) == tile).any():
            self._t("dp.two_in_tile")
        if (((later - 1) // TILE) > tile).any():
            self._t("dp.later_tile_candidate")
        hc = np.flatnonzero(cand[n])
        if A[n - 1, hc[0]] == A[n, hc[0]] or A[n + 1, hc[0]] == A[n, hc[0]]:
            self._t("dp.plateau")
        if A[n + 12, hc[0]] > A[n, hc[0]]:
            self._t("dp.no_veto_i12")
        if hc[0] > 0:
            self._t("dp.hit_channel_gt0")
        if A[n].max() > A[n, hc[0]]:   # the channel loop breaks at the first channel that hits
            self._t("dp.max_from_other_channel")
        self._veto_labels(A, samples, n)

    def _veto_labels(self, A, samples, upto):
        """three-point maxima above the ceiling before row `upto` whose only higher follower among i = 2..11 is i = 11"""
        tp, m = self.target_tp, min(upto, samples)
        if m < 2:
            return
        th = A[1:m]
        three = (A[0:m - 1] <= th) & (th >= A[2:m + 1]) & (th > tp)
        for n, c in zip(*np.nonzero(three)):
            higher = [i for i in range(2, 12) if A[n + 1 + i, c] > A[n + 1, c]]
            if higher == [11]:
                self._t("dp.veto_i11")

    # ------------------------------------------------------------------ gaussian filter
    def gaussian_filter(self, index):
        result = 0.0
        index = index - 10 if index > 10 else index + 20
        delta = self.delta[index:] + self.delta
        for weight, d in zip(self.weights, delta):
            result += d * weight
        return result


def detect_candidates(A, samples, target_tp):
    """(samples, ch) bool: rows n in [1, samples) where channel c passes detect_peak's test; A holds |x| of >= samples + 12 frames"""
    hit = np.zeros((samples, A.shape[1]), bool)
    if samples < 2:
        return hit
    th = A[1:samples]
    ok = (A[0:samples - 1] <= th) & (th >= A[2:samples + 1]) & (th > target_tp)
    for i in range(2, 12):
        ok &= ~(A[1 + i:samples + i] > th)
    hit[1:] = ok
    return hit


def detect_peak_serial(limiter_buf, channels, index, samples, target_tp, prev_smp, frame):
    """detect_peak (imp.rs:1438-1527), literally; `index` is the start already wrapped, `frame(i)` yields the element indices
    of limiter_buf[i..i + channels], prev_smp is updated in place"""
    llen = len(limiter_buf)
    for n in range(samples):
        next_index = index + channels
        if next_index >= llen:
            next_index -= llen
        this = [float(limiter_buf[i]) for i in frame(index)]
        next_ = [float(limiter_buf[i]) for i in frame(next_index)]
        detected = False
        for c in range(channels):
            t = abs(this[c])
            nx = abs(next_[c])
            detected = False
            if prev_smp[c] <= t and t >= nx and t > target_tp and n > 0:
                detected = True
                for i in range(2, 12):
                    ni = index + c + i * channels
                    if ni >= llen:
                        ni -= llen
                    if abs(float(limiter_buf[ni])) > t:
                        detected = False
                        break
                if detected:
                    break
            prev_smp[c] = t
        if detected:
            max_peak = 0.0
            for c in range(channels):
                if c == 0 or abs(this[c]) > max_peak:
                    max_peak = abs(this[c])
                prev_smp[c] = abs(this[c])
            return n, max_peak
        index = next_index
    return None


def init_gaussian_filter():
    weights = [0.0] * 21
    total = 0.0
    sigma = 3.5
    offset = 21 // 2
    c1 = 1.0 / (sigma * math.sqrt(2.0 * math.pi))
    c2 = 2.0 * math.pow(sigma, 2.0)
    for i in range(21):
        x = float(i) - float(offset)
        weights[i] = c1 * math.exp(-(math.pow(x, 2.0) / c2))
        total += weights[i]
    adjust = 1.0 / total
    for i in range(21):
        weights[i] *= adjust
    return weights
