"""Case builders shared by the mixer tests (tests/test_minus1mixer_cpu.py, tests/test_gpu_minus1mixer.py, tests/test_gpu_agroup_mixer.py).

A Case is what one interval of one mixer is made of: the contribution matrix, the segments in the order they are mixed, the outputs
and `frames`. expected() is the restatement's answer (tests/minus1mixer_restate.py), computed once per case."""
import numpy as np

import minus1mixer_restate as R

F32, S16 = R.F32, R.S16
FRAMES = 480                     # the reference tests' 10 ms at 48 kHz (tests/minus1mixer.rs:146-291)
SENTINEL_F32 = np.float32(-12345.5)
SENTINEL_S16 = np.int16(-12345)
FLT_MAX = np.float32(3.4028234663852886e38)


class Case:
    def __init__(self, contrib, segments, outputs, frames, name=""):
        """segments: (input, 1-D float32 / int16 array, out_offset); outputs: (format, channel_offset, n_channels)"""
        self.contrib = np.asarray(contrib, dtype=bool)
        self.segments, self.outputs, self.frames, self.name = list(segments), list(outputs), int(frames), name
        self._want = None

    @property
    def n_inputs(self):
        return self.contrib.shape[0]

    @property
    def n_out(self):
        return self.contrib.shape[1]

    def expected(self):
        if self._want is None:
            self._want = R.mix(self.contrib, self.segments, self.outputs, self.frames)
            for a in self._want:
                a.setflags(write=False)
        return self._want

    def buffers(self):
        """the caller's output arrays, pre-filled with a pattern no mix produces"""
        return [np.full(self.frames * nch, SENTINEL_S16 if fmt == S16 else SENTINEL_F32, R.DTYPE[fmt]) for fmt, _, nch in self.outputs]

    def call(self, bufs):
        """(segments, outputs) as mi355fx.mixer_tables takes them"""
        return self.segments, [(b, off, nch) for b, (_, off, nch) in zip(bufs, self.outputs)]


def untouched(bufs):
    return all((b == (SENTINEL_S16 if b.dtype == np.int16 else SENTINEL_F32)).all() for b in bufs)


def same(got, want):
    """bit for bit, except that an F32 sample that is NaN in the restatement only has to be NaN (payloads differ between machines)"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == np.float32:
        nan = np.isnan(want)
        return bool(np.isnan(got[nan]).all() and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
    return bool(np.array_equal(got, want))


def assert_same(gots, case):
    wants = case.expected()
    assert len(gots) == len(wants)
    for o, (g, w) in enumerate(zip(gots, wants)):
        if not same(g, w):
            bad = np.flatnonzero(g.view(np.uint32 if g.dtype == np.float32 else np.int16) != w.view(np.uint32 if w.dtype == np.float32 else np.int16))
            i = int(bad[0]) if len(bad) else -1
            raise AssertionError("%s: output %d differs at sample %d: got %r, want %r" % (case.name, o, i, g[i], w[i]))


# ---------------------------------------------------------------- the reference's own vectors

def reference_vectors(in_fmt, out_fmt):
    """minus1mixer_direct_link_*: three inputs filled with 1 / 10 / 100 -> 110, 101, 11"""
    dt = R.DTYPE[in_fmt]
    segs = [(i, np.full(FRAMES, v, dt), 0) for i, v in enumerate((1, 10, 100))]
    return Case(R.minus1(3), segs, [(out_fmt, o, 1) for o in range(3)], FRAMES, "reference 1/10/100")


def reference_answer(in_fmt, out_fmt):
    """what the reference's tests assert, in the output's own unit: F32 in -> values as they are; S16 in -> v / 32768"""
    want = np.array([110, 101, 11], np.float64)
    if in_fmt == S16 and out_fmt == F32:
        want = want / 32768.0
    if in_fmt == F32 and out_fmt == S16:
        want = np.clip(want * 32768.0, -32768, 32767)
    return want


# ---------------------------------------------------------------- hand-worked values: inputs in order into ONE channel

def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


# (name, input values in mixing order, expected f32 bits of the sum (None: NaN), expected S16 of the sum)
SPECIALS = [
    ("big first", np.array([1e8, 1.0, -1e8], np.float32), 0x00000000, 0),                  # (1e8 + 1) rounds to 1e8
    ("big cancels first", np.array([1e8, -1e8, 1.0], np.float32), 0x3F800000, 32767),    # 1.0 -> 32768 saturates
    ("minus zero alone", np.array([-0.0], np.float32), 0x00000000, 0),                     # +0.0 + -0.0 = +0.0
    ("s16 top", np.array([32767, 32767], np.int16), 0x3FFFFE00, 32767),                    # 65534 / 32768
    ("s16 bottom", np.array([-32768, -32768], np.int16), 0xC0000000, -32768),              # -2.0
    ("toward zero", np.array([-0.5 / 32768, -0.25 / 32768], np.float32), 0xB7C00000, 0),   # -0.75 / 32768 -> -0.75 -> 0, not -1
    ("inf minus inf", np.array([np.inf, -np.inf], np.float32), None, 0),
    ("overflow", np.array([FLT_MAX, FLT_MAX], np.float32), 0x7F800000, 32767),
    ("denormals", np.array([_bits(1), _bits(2)], np.float32), 0x00000003, 0),
]


def special_case(values, frames=1, at=(0,), filler=None):
    """every value is an input of its own; all feed channel 0, which an F32 and an S16 output both own. The values sit at the frames
    `at`; the other frames carry `filler` (a value per input, default 0)."""
    n = len(values)
    segs = []
    for i, v in enumerate(values):
        d = np.full(frames, 0 if filler is None else filler[i], values.dtype)
        d[list(at)] = v
        segs.append((i, d, 0))
    return Case(np.ones((n, 1), bool), segs, [(F32, 0, 1), (S16, 0, 1)], frames, "special")


# ---------------------------------------------------------------- random material

def samples(rng, fmt, n):
    if fmt == S16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return (rng.standard_normal(n) * 0.4).astype(np.float32)


def random_minus1(seed, n, frames, name=None):
    """n participants, a whole-interval segment each, segment and output formats mixed within the call"""
    rng = np.random.default_rng(seed)
    segs = [(i, samples(rng, int(rng.integers(0, 2)), frames), 0) for i in range(n)]
    outs = [(int(rng.integers(0, 2)), o, 1) for o in range(n)]
    if n >= 2:   # both formats on both sides whatever the draw
        segs[0] = (0, samples(rng, F32, frames), 0)
        segs[1] = (1, samples(rng, S16, frames), 0)
        outs[0], outs[1] = (S16, 0, 1), (F32, 1, 1)
    return Case(R.minus1(n), segs, outs, frames, name or "minus1 n=%d frames=%d" % (n, frames))


def random_general(seed, n_in, n_out, frames):
    """a random matrix with one channel nobody feeds; outputs of 1 and 2 channels, overlapping, and channels no output owns"""
    rng = np.random.default_rng(seed)
    contrib = rng.integers(0, 2, (n_in, n_out)).astype(bool)
    silent = n_out // 2
    contrib[:, silent] = False
    segs = [(i, samples(rng, int(rng.integers(0, 2)), frames), 0) for i in range(n_in)]
    outs = [(S16, silent, 1), (F32, silent, 1)]
    c = 0
    while c + 2 <= n_out:
        outs.append((int(rng.integers(0, 2)), c, 2))          # a stereo output ...
        outs.append((int(rng.integers(0, 2)), c + 1, 1))      # ... and a mono one on its second channel (overlap)
        c += 5                                                # channels c + 2 .. c + 4 belong to nobody (sparse)
    outs.append((F32, n_out - 1, 1))
    return Case(contrib, segs, outs, frames, "general %dx%d frames=%d" % (n_in, n_out, frames))
