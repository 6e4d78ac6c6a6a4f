"""The staging of the audio groups (csrc/agroup.hip: the slabs, the host runs, the copies in and out) held where the kinds share it:
a result that has run and has not been collected lies in its row while ANOTHER launch set of the group runs around it and while
a larger buffer replaces the slabs. Every member's output - and its carried state where the kind exposes it - is numpy.array_equal
to a lone Context fed the same buffers. A characterization: it passes against the library of the commit before the staging was
unified (MI355FX_LIB selects a library) and against this one.

The common case, six members, linger 0, one thread, three rounds in one group so that state carries across sets:
  set A  member 2 (host) and member 0 (host) submit; member 0 waits, which runs the set, and collects. Member 2 does not collect.
         (Only a member's outstanding ticket runs a set: wait refuses every other ticket before it touches anything, so a second
         member has to come along, as in test_gpu_agroup.py::test_echo_results_survive_a_growing_slab.)
  set B  members 0, 1, 3 (host, small), 4 (device buffers) and 5 (host, larger than the slots: both slabs are replaced) submit.
         The set's host runs are {0, 1}, {3} and {5}; member 2's uncollected row lies between two of them, in fresh slabs.
  collect in the order 0, 2, 5, 1, 3, 4.
Member 5's buffer crosses the slot size of the round before in every round (sizes worked out at each kind below; slots are powers
of two from 4096 bytes)."""
import numpy as np
import pytest

import agingradio_restate as AR
import audio_state_cases as A
import hrtf_group_cases as H
import minus1mixer_cases as M
import minus1mixer_restate as MR
import mi355fx

pytestmark = pytest.mark.gpu

N = 6
DEVICE, BIG, PENDING = 4, 5, 2
ROUNDS = 3


def _noise(seed, shape, dtype=np.float32, scale=0.5):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(dtype)


class _Kind:
    """one group of N members, their lone contexts and a context that owns the device member's buffers"""

    def __init__(self, kind, **kw):
        self.g = mi355fx.AudioGroup(kind, N, **kw)
        self.lone = [mi355fx.Context(0) for _ in range(N)]
        self.dev = mi355fx.Context(0)
        self.held = []
        self.g.set_linger(0)

    def before_round(self, r):
        pass

    def to_device(self, a):
        p = self.dev.alloc(max(a.nbytes, 16))
        self.held.append(p)
        self.dev.h2d(p, a)
        self.dev.synchronize()
        return p

    def from_device(self, p, like):
        out = np.empty_like(like)
        self.dev.d2h(out, p)
        return out

    def states(self):
        return []

    def close(self):
        for p in self.held:
            self.dev.free(p)
        self.g.close()
        for c in self.lone + [self.dev]:
            c.close()


class _Echo(_Kind):
    """small: 300 + m f32 samples (1.2 KB: 4 KiB slots). Member 5: 2400, 9600, 38400 f64 samples = 19,200 B (32 KiB slots), 76,800 B
    (128 KiB; above the 64 KiB from which a buffer is copied outside the lock) and 307,200 B (512 KiB)."""
    RING = 4096
    PAR = [(1000, 0.5, 0.3), (0, 0.5, 0.0), (RING, 0.3, 0.9), (7, 0.25, 0.25), (96, 0.8, 0.0), (777, 0.25, 0.0)]

    def __init__(self, synth):
        super().__init__("echo", ring_len=self.RING)
        for c in self.lone:
            c.echo_setup(self.RING)

    def buf(self, m, r, seed, big):
        return _noise(seed, 600 * 4 ** (r + 1), np.float64) if big else _noise(seed, 300 + m)

    def want(self, m, x):
        return [self.lone[m].echo_process(x.copy(), *self.PAR[m])]

    def submit(self, m, x, device):
        if device:
            p = self.to_device(x)
            return self.g.submit_echo(m, p, *self.PAR[m], n=x.size, is_f64=x.dtype == np.float64), p
        y = x.copy()
        return self.g.submit_echo(m, y, *self.PAR[m]), y

    def got(self, m, x, h, device, frames):
        assert frames == x.size
        return [self.from_device(h, x) if device else h]

    def states(self):
        out = []
        for m in range(N):
            (r1, p1), (r0, p0) = self.g.echo_state(m, self.RING), self.lone[m].echo_state(self.RING)
            out.append((np.append(r1, p1), np.append(r0, p0)))
        return out


class _Aging(_Kind):
    """two channels. small: 100 + m frames f32 (0.8 KB). Member 5: 1200, 4800, 19200 frames f64 = the byte sizes of the echo case."""
    CH, RATE = 2, 48000
    LOWPASS = [2000, 0, 1, 2000, 0, 22000]

    def __init__(self, synth):
        super().__init__("agingradio")
        for m in range(N):
            self.g.agingradio_setup(m, self.CH, self.RATE, self.LOWPASS[m], 900 + m)
            self.lone[m].agingradio_setup(self.CH, self.RATE, self.LOWPASS[m], 900 + m)

    def settings(self, m):
        return dict(AR.DEFAULTS, lowpass_freq=self.LOWPASS[m])

    def buf(self, m, r, seed, big):
        frames, dtype = (300 * 4 ** (r + 1), np.float64) if big else (100 + m, np.float32)
        return np.random.default_rng(seed).uniform(-1.2, 1.2, frames * self.CH).astype(dtype)

    def want(self, m, x):
        return [self.lone[m].agingradio_process(x.copy(), self.CH, self.settings(m))]

    def submit(self, m, x, device):
        if device:
            p = self.to_device(x)
            return self.g.submit_agingradio(m, p, self.settings(m), frames=x.size // self.CH, is_f64=x.dtype == np.float64), p
        y = x.copy()
        return self.g.submit_agingradio(m, y, self.settings(m), channels=self.CH), y

    def got(self, m, x, h, device, frames):
        assert frames == x.size // self.CH
        return [self.from_device(h, x) if device else h]

    def states(self):
        out = []
        for m in range(N):
            (y1, k1), (y0, k0) = self.g.agingradio_state(m, self.CH), self.lone[m].agingradio_state(self.CH)
            out.append((np.append(y1, k1), np.append(y0, k0)))
        return out


class _Hrtf(_Kind):
    """three channels, four interpolation steps. small: block-length 128 = 512 frames, 6 KB in (8 KiB slots) and 4 KB out (4 KiB).
    A member's block is fixed by its setup, so member 5 is set up anew before every round, its lone context with it: block-length
    256, 512, 2048 = 12 KB, 24 KB, 96 KB in (16, 32, 128 KiB slots) and 8, 16, 64 KB out. The other members carry their tails on."""
    CFG = dict(file_len=256, file_rate=44100, rate=44100, len=256, channels=3, steps=4, block=128, method=0)
    BIG_BLOCKS = [256, 512, 2048]

    def __init__(self, synth):
        super().__init__("hrtf")
        sp = H.sphere_bytes(synth, self.CFG)
        self.cfg = [dict(self.CFG) for _ in range(N)]
        for m in range(N):
            self.g.hrtf_load_sphere(m, sp, self.CFG["rate"])
            self.lone[m].hrtf_load_sphere(sp, self.CFG["rate"])
            self.setup(m, self.CFG["block"])

    def setup(self, m, block):
        c = self.cfg[m]
        c["block"] = block
        self.g.hrtf_setup(m, c["channels"], block, c["steps"], 0)
        self.lone[m].hrtf_setup(c["channels"], block, c["steps"])

    def before_round(self, r):
        self.setup(BIG, self.BIG_BLOCKS[r])

    def buf(self, m, r, seed, big):
        return H.stream(self.cfg[m], 1, seed=seed)[0]

    def want(self, m, b):
        return [self.lone[m].hrtf_process_block(*b).copy()]

    def submit(self, m, b, device):
        x, pos, gains = b
        if device:
            p, q = self.to_device(x), self.to_device(np.zeros(x.shape[0] * 2, np.float32))
            return self.g.submit_hrtf(m, p, pos, gains, out=q), q
        return self.g.submit_hrtf(m, x, pos, gains), None

    def got(self, m, b, h, device, frames):
        assert frames == b[0].shape[0]
        return [self.from_device(h, np.zeros(frames * 2, np.float32)) if device else self.g.hrtf_output(m).copy()]

    def states(self):
        out = []
        for m in range(N):
            (f1, w1), (f0, w0) = self.g.hrtf_last_lookup(m), self.lone[m].hrtf_last_lookup()
            out += [(f1, f0), (w1, w0)]
        return out


class _Sofa(_Kind):
    """two channels, 128 taps, partition-length 64. small: one block of 256 frames, 2 KB in and out (4 KiB slots). Member 5:
    block-length 512 and 2, 4, 8 blocks per submit (8 is the most a submit takes) = 8, 16, 32 KB in and out."""
    SHAPE, BIG_SHAPE = (2, 128, 64, 256), (2, 128, 64, 512)
    BIG_BLOCKS = [2, 4, 8]

    def __init__(self, synth):
        super().__init__("sofa")
        self.shape = [self.BIG_SHAPE if m == BIG else self.SHAPE for m in range(N)]
        for m in range(N):
            self.g.sofa_setup(m, *self.shape[m])
            self.lone[m].sofa_setup(*self.shape[m])
            for c, (l, r) in enumerate(A.sofa_filters(np.random.default_rng(40 + m), 2, 128)):
                self.g.sofa_set_filter(m, c, l, r, c, 2 * c)
                self.lone[m].sofa_set_filter(c, l, r, c, 2 * c)

    def buf(self, m, r, seed, big):
        C, _, _, B = self.shape[m]
        nb = self.BIG_BLOCKS[r] if big else 1
        return _noise(seed, (nb * B, C)), np.random.default_rng(seed).uniform(0.2, 1.0, C).astype(np.float32), nb

    def want(self, m, b):
        x, gains, nb = b
        B = self.shape[m][3]
        return [np.concatenate([self.lone[m].sofa_process_block(x[i * B:(i + 1) * B], gains) for i in range(nb)]).reshape(-1)]

    def submit(self, m, b, device):
        x, gains, nb = b
        if device:
            p, q = self.to_device(x), self.to_device(np.zeros(x.shape[0] * 2, np.float32))
            return self.g.submit_sofa(m, p, gains, n_blocks=nb, out=q), q
        return self.g.submit_sofa(m, x, gains, n_blocks=nb), None

    def got(self, m, b, h, device, frames):
        assert frames == b[0].shape[0]
        return [self.from_device(h, np.zeros(frames * 2, np.float32)) if device else self.g.sofa_output(m).reshape(-1).copy()]


class _Mixer(_Kind):
    """a member is a minus-1 room with one segment and one output per party, S16 (2 B a sample) and F32 (4 B) mixed, at least one
    F32 on either side. small: 3 parties, 48 + m frames, at most 0.6 KB in and out (4 KiB slots). Member 5: 8 parties and 512,
    1024, 4096 frames: between 9 and 16 KB, 18 and 32 KB, 72 and 128 KB in and out - each above the slots the round before can have
    left (16 KiB, 32 KiB), the last above the 64 KiB from which the segments are copied outside the lock. Stateless between intervals."""
    BIG_FRAMES = [512, 1024, 4096]

    def __init__(self, synth):
        super().__init__("mixer")

    def buf(self, m, r, seed, big):
        return M.random_minus1(seed, 8, self.BIG_FRAMES[r]) if big else M.random_minus1(seed, 3, 48 + m)

    def want(self, m, case):
        self.lone[m].mixer_setup(case.contrib)
        bufs = case.buffers()
        self.lone[m].mixer_process(*case.call(bufs), case.frames)
        return bufs

    def submit(self, m, case, device):
        self.g.mixer_setup(m, case.contrib)
        bufs = case.buffers()
        if not device:
            return self.g.submit_mixer(m, *case.call(bufs), case.frames), bufs
        segs = [(inp, (self.to_device(data), MR.fmt_of(data), data.size), off) for inp, data, off in case.segments]
        outs = [((self.to_device(b), fmt), off, nch) for b, (fmt, off, nch) in zip(bufs, case.outputs)]
        return self.g.submit_mixer(m, segs, outs, case.frames, device_data=True), (bufs, outs)

    def got(self, m, case, h, device, frames):
        assert frames == case.frames
        if not device:
            return h
        bufs, outs = h
        return [self.from_device(pf[0], b) for b, (pf, _, _) in zip(bufs, outs)]

    def states(self):
        assert self.g.mixer_launches() == 2 * ROUNDS   # one kernel launch per launch set
        return []


def _equal(gots, wants, what):
    assert len(gots) == len(wants), what
    for o, (got, want) in enumerate(zip(gots, wants)):
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, o, got.dtype, want.dtype, got.shape, want.shape)
        assert np.array_equal(got, want), (what, o, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("kind", [_Echo, _Aging, _Hrtf, _Sofa, _Mixer], ids=["echo", "agingradio", "hrtf", "sofa", "mixer"])
def test_an_uncollected_result_between_the_runs_of_a_set_in_fresh_slabs(mi355lib, synth, kind):
    k = kind(synth)
    try:
        g = k.g
        for r in range(ROUNDS):
            k.before_round(r)
            seed = 1000 * (r + 1)
            # set A = {2, 0}: run by member 0's wait; member 2's result stays in the slabs
            a = {m: k.buf(m, r, seed + m, False) for m in (PENDING, 0)}
            want_a = {m: k.want(m, a[m]) for m in a}
            sub_a = {m: k.submit(m, a[m], False) for m in (PENDING, 0)}
            _equal(k.got(0, a[0], sub_a[0][1], False, g.wait(sub_a[0][0])), want_a[0], (r, "A", 0))
            assert g.stats() == (7 * r + 2, 2 * r + 1, 5 if r else 2)
            # set B = {0, 1, 3, 4, 5}: member 5's buffer replaces both slabs with member 2's result in them
            who = (0, 1, 3, DEVICE, BIG)
            b = {m: k.buf(m, r, seed + 100 + m, m == BIG) for m in who}
            want_b = {m: k.want(m, b[m]) for m in who}
            sub_b = {m: k.submit(m, b[m], m == DEVICE) for m in who}
            assert g.stats()[1] == 2 * r + 1                 # member 2 is not there: nothing has run yet
            for m in (0, PENDING, BIG, 1, 3, DEVICE):
                if m == PENDING:
                    _equal(k.got(m, a[m], sub_a[m][1], False, g.wait(sub_a[m][0])), want_a[m], (r, "A", m))
                else:
                    _equal(k.got(m, b[m], sub_b[m][1], m == DEVICE, g.wait(sub_b[m][0])), want_b[m], (r, "B", m))
            assert g.stats() == (7 * (r + 1), 2 * (r + 1), 5)
        for i, (got, want) in enumerate(k.states()):
            _equal([got], [want], ("state", i))
    finally:
        k.close()


def test_ebur128_host_runs_around_a_device_member_and_an_absent_one(mi355lib):
    """ebur128level has no download. Members: host, device, host, absent, host, one sample format (f32, two channels): the host runs
    of every set are {0}, {2} and {4}. Three intervals of ragged sizes; the largest host buffer of an interval is 5.6 KB (8 KiB
    slots), 76,800 B (128 KiB, copied in outside the lock) and 153,600 B (256 KiB): the slab is replaced twice with submissions in
    it. Every answer == a lone meter's; the absent member's == those of a meter that was never fed."""
    rate, ch, n = 48000, 2, 5
    sizes = [{0: 480, 1: 1000, 2: 333, 4: 700}, {0: 4801, 1: 480, 2: 100, 4: 9600}, {0: 333, 1: 4800, 2: 19200, 4: 7}]
    g = mi355fx.AudioGroup("ebur128", n, channels=ch, rate=rate, mode=63)
    lone = [mi355fx.Context(0) for _ in range(n)]
    dev = mi355fx.Context(0)
    held = []
    try:
        g.set_linger(0)
        for c in lone:
            c.ebur128_setup(ch, rate, 63)
        fed = [0] * n
        for it, frames in enumerate(sizes):
            tickets = {}
            for m in (4, 1, 0, 2):
                t = (fed[m] + np.arange(frames[m])) / rate
                x = np.stack([0.05 * (m + 1) * np.sin(2 * np.pi * (300.0 + 50 * m + 7 * c) * t) for c in range(ch)], 1)
                x = np.ascontiguousarray((x + 1e-3 * np.random.default_rng(10 * it + m).standard_normal(x.shape)).astype(np.float32)).reshape(-1)
                fed[m] += frames[m]
                lone[m].ebur128_add_frames(x)
                if m == 1:
                    held.append(dev.alloc(x.nbytes))
                    dev.h2d(held[-1], x)
                    dev.synchronize()
                    tickets[m] = g.submit_ebur128(m, held[-1], frames[m], 2)
                else:
                    tickets[m] = g.submit_ebur128(m, x)
            for m in (0, 1, 2, 4):
                assert g.wait(tickets[m]) == frames[m]
            assert g.stats() == (4 * (it + 1), it + 1, 4)
        for m in range(n):
            s = lone[m]
            own = [s.ebur128_loudness_momentary(), s.ebur128_loudness_shortterm(), s.ebur128_loudness_global(), s.ebur128_relative_threshold(), s.ebur128_loudness_range()]
            got = [g.loudness(m, what) for what in range(5)]
            assert np.array_equal(np.array(got), np.array(own)), (m, got, own)
            for c in range(ch):
                assert g.peak(m, c) == s.ebur128_sample_peak(c) and g.peak(m, c, True) == s.ebur128_true_peak(c), (m, c)
    finally:
        for p in held:
            dev.free(p)
        g.close()
        for c in lone + [dev]:
            c.close()


def _loudnorm_signal(seed, frames, ch):
    t = np.arange(frames) / 192000
    x = np.stack([0.05 * np.sin(2 * np.pi * (440 + 13 * seed + 3 * c) * t) * (1 + 0.5 * np.sin(2 * np.pi * 0.2 * t)) for c in range(ch)], 1)
    rng = np.random.default_rng(seed)
    for s in rng.uniform(0.3, frames / 192000 - 0.3, 5):
        i = int(s * 192000)
        x[i:i + int(rng.integers(10, 3000))] *= rng.uniform(10, 25)
    return x


def test_loudnorm_pending_row_between_two_classes_at_three_channels(mi355lib):
    """audioloudnorm at THREE channels: an output row (the slot rounded down to whole frames of 24 bytes) is not the slot width.
    Four members; the slabs are sized at create and do not grow at this member count, so this covers the uncollected result between
    the runs of a set, and the classes. Members 0 and 1 (host) and 2 (device buffers) start together with their 3 s frames; then,
    three times:
      set A  members 1 and 0 hand over a 100 ms frame; member 0's wait runs the set; member 1 does not collect.
      set B  members 0 (host), 2 (device) and 3 (host) hand over their next frame - member 3 starts late: its 3 s first frame is a
             class of its own beside the others' 100 ms frames in the first round. Host runs {0} and {3}, member 1's row between.
      collect 0, 1, 3, 2.
    Then everybody hands over its rest as the final frame. Samples == lone instances pushed the same signal and drained."""
    ch, n, F = 3, 4, 19200
    lengths = [576000 + 6 * F + 5000, 576000 + 3 * F + 777, 576000 + 3 * F + 1, 576000 + 2 * F + 12345]
    xs = [_loudnorm_signal(60 + m, lengths[m], ch) for m in range(n)]
    want = []
    for x in xs:
        c = mi355fx.Context(0)
        c.loudnorm_setup(ch)
        parts = [c.loudnorm_push(x)]
        d = c.loudnorm_drain()
        want.append(np.concatenate(parts + ([d] if d is not None else [])))
        c.close()
    g = mi355fx.AudioGroup("loudnorm", n, channels=ch)
    dev = mi355fx.Context(0)
    d_in, d_out = dev.alloc(576000 * ch * 8), dev.alloc(31 * F * ch * 8)
    try:
        g.set_linger(0)
        pos, outs = [0] * n, [[] for _ in range(n)]

        def submit(m, final=False):
            fs = g.loudnorm_frame_size(m)
            x = xs[m][pos[m]:] if final else xs[m][pos[m]:pos[m] + fs]
            assert final or len(x) == fs
            pos[m] += len(x)
            cap = 31 * F if final else max(fs, F)
            if m == 2:
                dev.h2d(d_in, x)
                dev.synchronize()
                return g.submit_loudnorm(m, d_in, d_out, final_frame=final, frames=len(x), out_capacity_frames=cap), None
            out = np.zeros((cap, ch))
            return g.submit_loudnorm(m, x, out, final_frame=final), out

        def collect(m, sub):
            t, out = sub
            frames = g.wait(t)
            if m == 2:
                out = np.zeros((frames, ch))
                if frames:
                    dev.d2h(out, d_out)
            outs[m].append(out[:frames].reshape(-1).copy())

        first = {m: submit(m) for m in (0, 1, 2)}        # three 3 s first frames, one class; member 3 has not come
        for m in (0, 1, 2):
            collect(m, first[m])
        for r in range(3):
            a = {m: submit(m) for m in (1, 0)}
            collect(0, a[0])
            b = {m: submit(m) for m in (0, 2, 3)}
            collect(0, b[0])
            collect(1, a[1])
            collect(3, b[3])
            collect(2, b[2])
        last = {m: submit(m, final=True) for m in range(n)}
        for m in (3, 0, 2, 1):
            collect(m, last[m])
        assert g.stats() == (3 + 3 * 5 + 4, 1 + 3 * 2 + 1, 4)
        for m in range(n):
            got = np.concatenate(outs[m])
            assert got.size == want[m].size, (m, got.size, want[m].size)
            assert np.array_equal(got, want[m]), (m, int(np.flatnonzero(got != want[m])[0]))
    finally:
        dev.free(d_in)
        dev.free(d_out)
        g.close()
        dev.close()
