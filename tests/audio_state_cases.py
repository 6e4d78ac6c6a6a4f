"""Signal builders and pure-numpy references for the carried-state tests of the audio elements
(tests/test_gpu_audio_state.py, tests/test_gpu_sofa.py, CPU checks in tests/test_audio_state_cpu.py).

Everything here is generated from seeds; nothing reads a file. The builders put the quantity under test ON a cut the kernels
make (buffer edge, 256-frame chunk, ring wrap, partition slot), so that a state carried wrongly by one position decides the
reading instead of hiding in the tail of seconds of programme."""
import numpy as np

FLOOR = 1e-3            # -60 dBFS: the floor every event stands on
EB_RATES = (44100, 48000, 96000, 192000)


def eb_delay(rate):
    """taps per phase of the 49-tap true-peak interpolator = samples of history the meter keeps per channel (0: no interpolator)"""
    return 13 if rate < 96000 else 25 if rate < 192000 else 0


# ---------------------------------------------------------------- ebur128: true peak at the buffer edge

EB_LEAD = 160           # frames before the reference position of the events


def tp_shifts(rate, channels):
    """offset of every channel's event from the reference position E0: a different place per channel, delay - 3 frames apart, so
    that with four channels every cut within +-delay of E0 has an event whose interpolated peak draws on frames from both sides
    of it (the peak of an event at E comes out half a filter later and rests on about half a filter to either side of E)"""
    d = max(eb_delay(rate), 13)
    return [-d - 3 + (d - 3) * (c % 4) + c // 4 for c in range(channels)]


def tp_stream(rate, channels, seed=0):
    """(frames, channels) f64: seeded floor at -60 dBFS, one inter-sample over per channel near frame EB_LEAD: an equal-sign
    doublet on even channels (the x4 / x2 peak lies between the two samples and draws on taps from both sides), a triple of the
    other sign on odd ones. Returns (stream, floor alone, list of the event's frame indices per channel)."""
    rng = np.random.default_rng(1000 + seed + rate % 1013)
    d = max(eb_delay(rate), 13)
    n = EB_LEAD + 6 * d + 40
    floor = FLOOR * rng.uniform(-1.0, 1.0, (n, channels))
    x = floor.copy()
    where = []
    for c, s in enumerate(tp_shifts(rate, channels)):
        e = EB_LEAD + s
        if c % 2 == 0:
            x[e:e + 2, c] = [-0.97, -0.96]
            where.append([e, e + 1])
        else:
            x[e:e + 3, c] = [0.9, 0.93, 0.9]
            where.append([e, e + 1, e + 2])
    return x, floor, where


def tp_format(x, where, dtype):
    """the stream in one of the four sample formats; the integer formats carry their minimum (exactly -1.0) as the first event sample"""
    if dtype == np.int16:
        y = np.round(x * 32767.0).astype(np.int16)
        for c, w in enumerate(where):
            y[w[0], c] = -32768
        return y
    if dtype == np.int32:
        y = np.round(x * 2147483647.0).astype(np.int64)
        for c, w in enumerate(where):
            y[w[0], c] = -2147483648
        return y.astype(np.int32)
    return x.astype(dtype)


def tp_cuts(rate):
    """every position of the cut from -delay to +delay around the events' reference position"""
    d = max(eb_delay(rate), 13)
    return [EB_LEAD + o for o in range(-d, d + 1)]


def tp_short_schedules(rate, frames):
    """buffer-size lists: a long lead, then runs of 1, 2, delay-1, delay, delay+1 frame buffers up to and across the events, then
    one long buffer (the n < delay path of the history update and the path just above it)"""
    d = max(eb_delay(rate), 13)
    out = []
    for s in (1, 2, d - 1, d, d + 1):
        sizes, pos = [EB_LEAD - 3 * d - 5], EB_LEAD - 3 * d - 5
        while pos < EB_LEAD + 3 * d:
            sizes.append(s)
            pos += s
        sizes.append(frames - pos)
        out.append(sizes)
    return out


def split(x, sizes):
    """consecutive row blocks of x with the given sizes"""
    out, pos = [], 0
    for s in sizes:
        out.append(x[pos:pos + s])
        pos += s
    assert pos == len(x)
    return out


# ---------------------------------------------------------------- ebur128: K-weighting impulse response (independent f64 reference)

def kweight_impulse_energy(b, a, n, shift_state_at=None):
    """sum of squares of the first n samples of the impulse response of the 4th-order K-weighting filter, plain direct form II:
    v0 = x - a1 v1 - a2 v2 - a3 v3 - a4 v4;  y = b0 v0 + b1 v1 + b2 v2 + b3 v3 + b4 v4
    shift_state_at: sample in front of which the four carried values slip by one position (what a wrong carry does; only the
    CPU companion uses it, to show that the reading notices)"""
    v = [0.0, 0.0, 0.0, 0.0]
    e = 0.0
    for i in range(n):
        if i == shift_state_at:
            v = [v[1], v[2], v[3], 0.0]
        x = 1.0 if i == 0 else 0.0
        v0 = x - a[1] * v[0] - a[2] * v[1] - a[3] * v[2] - a[4] * v[3]
        y = b[0] * v0 + b[1] * v[0] + b[2] * v[1] + b[3] * v[2] + b[4] * v[3]
        v = [v0, v[0], v[1], v[2]]
        e += y * y
    return e


# (buffer sizes, absolute frame of the impulse): frames 255 / 256 / 257 of a buffer (the 256-frame chunk of the filter kernel), the
# last frame of a buffer, a 1-frame buffer; the zeros that follow keep the impulse inside the 400 ms window
IMPULSE_CASES = [([600, 3000], 255), ([600, 3000], 256), ([600, 3000], 257), ([40, 600, 3000], 40 + 255), ([300, 3000], 299),
                 ([513, 3000], 512), ([100, 1, 3000], 100), ([1, 1, 1, 3000], 1)]
IMPULSE_RATE = 48000
IMPULSE_CLASSES = [1, 0, 1]       # a class-0 (unused) channel between two used ones
IMPULSE_AMPL = [1.0, 0.75, 0.5]   # the unused channel carries an impulse of its own one frame later: it must not count


def impulse_stream(sizes, pos):
    x = np.zeros((sum(sizes), 3))
    x[pos, 0], x[pos + 1, 1], x[pos, 2] = IMPULSE_AMPL
    return x


def impulse_momentary(b, a, sizes, pos, rate=IMPULSE_RATE):
    """momentary loudness after the whole stream: the 400 ms energy is the squared impulse response"""
    n = sum(sizes) - pos
    window = 4 * ((rate + 5) // 10)
    assert sum(sizes) <= window
    e = kweight_impulse_energy(b, a, n) * (IMPULSE_AMPL[0] ** 2 + IMPULSE_AMPL[2] ** 2)
    return 10.0 * np.log10(e / window) - 0.691


# ---------------------------------------------------------------- sofalizer: float32 restatement of the partitioned overlap-save

def fft32(x, inverse=False):
    """radix-2 decimation-in-time transform along the last axis, complex64 throughout (f32 twiddles, f32 butterflies), unscaled"""
    x = np.asarray(x, np.complex64)
    n = x.shape[-1]
    bits = n.bit_length() - 1
    assert 1 << bits == n
    idx = np.arange(n)
    rev = np.zeros(n, np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    a = np.ascontiguousarray(x[..., rev])
    lead = a.shape[:-1]
    half = 1
    while half < n:
        w = np.exp((2j if inverse else -2j) * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        a = a.reshape(lead + (n // (2 * half), 2, half))
        top, bot = a[..., 0, :], (a[..., 1, :] * w).astype(np.complex64)
        a = np.stack([top + bot, top - bot], axis=-2).astype(np.complex64).reshape(lead + (n,))
        half *= 2
    return a


class SofaF32:
    """The device's algorithm restated in numpy float32: uniformly partitioned overlap-save, partition P, transform 2P,
    K = ceil(L / P) filter partitions, frequency-domain delay line, partitions summed in ascending order, channel-ordered mix."""

    def __init__(self, channels, filter_len, partition, block):
        self.C, self.L, self.P, self.B = channels, filter_len, partition, block
        self.K, self.N = -(-filter_len // partition), 2 * partition
        self.H = np.zeros((channels, 2, self.K, self.N), np.complex64)
        self.drop = [False] * channels
        self.reset()

    def reset(self):
        self.fdl = np.zeros((self.C, self.K, self.N), np.complex64)
        self.prev = np.zeros((self.C, self.P), np.float32)
        self.counter = 0

    def set_filter(self, c, left, right, delay_left=0, delay_right=0):
        for e, (h, d) in enumerate(((left, delay_left), (right, delay_right))):
            t = np.zeros(self.K * self.P, np.float32)
            if self.L - d > 0:
                t[d:self.L] = np.asarray(h, np.float32)[:self.L - d]
            parts = np.concatenate([t.reshape(self.K, self.P), np.zeros((self.K, self.P), np.float32)], axis=1)
            self.H[c, e] = fft32(parts)

    def process_block(self, block, gains):
        x = np.asarray(block, np.float32).reshape(self.B, self.C)
        partial = np.zeros((self.C, self.B, 2), np.float32)
        for j in range(self.B // self.P):
            slot = self.counter % self.K
            cur = np.ascontiguousarray(x[j * self.P:(j + 1) * self.P].T)
            X = fft32(np.concatenate([self.prev, cur], axis=1))
            self.prev = cur
            self.fdl[:, slot] = X
            for e in range(2):
                acc = np.zeros((self.C, self.N), np.complex64)
                for k in range(self.K):
                    acc = (acc + self.fdl[:, (slot - k) % self.K] * self.H[:, e, k]).astype(np.complex64)
                y = fft32(acc, inverse=True).real.astype(np.float32) * np.float32(1.0 / self.N)
                partial[:, j * self.P:(j + 1) * self.P, e] = y[:, self.P:]
            self.counter += 1
        out = np.zeros((self.B, 2), np.float32)
        for c in range(self.C):
            if not self.drop[c]:
                out = (out + partial[c] * np.float32(gains[c])).astype(np.float32)
        return out


def sofa_filters(rng, channels, L):
    k = np.arange(L)
    env = np.exp(-k / (0.1 * L + 4.0))
    return [((0.5 * env * rng.standard_normal(L)).astype(np.float32), (0.4 * env * rng.standard_normal(L)).astype(np.float32))
            for _ in range(channels)]


# (channels, L, P, B): the partition sizes at both ends of what setup accepts (8 and 2048), 512 and 1024 with B = P and B = 2P, one
# partition with L < P and L == P, L == P + 1 (one live tap in the second partition), 64 channels, B / P coprime to K (3 sub-blocks
# per block against 5 slots: every slot starts a block within 5 blocks)
SOFA_NEW_SHAPES = [(2, 20, 8, 8), (2, 50, 8, 64), (2, 1500, 512, 512), (1, 1024, 512, 1024), (1, 2048, 1024, 1024), (2, 1024, 1024, 2048),
                   (1, 3000, 2048, 2048), (2, 2049, 2048, 4096), (2, 10, 16, 32), (2, 16, 16, 16), (2, 17, 16, 48), (64, 40, 16, 32),
                   (2, 80, 16, 48)]

# worst |float32 restatement - f64 time domain| / max(1, max|f64|) over sofa_run, measured on the CPU (test_audio_state_cpu.py
# recomputes every figure and fails if one is off by more than a factor of two); the device is held to twice the figure
SOFA_F32_ERR = {
    (2, 20, 8, 8): 1.14e-7, (2, 50, 8, 64): 2.04e-7, (2, 1500, 512, 512): 2.06e-7, (1, 1024, 512, 1024): 2.18e-7,
    (1, 2048, 1024, 1024): 2.11e-7, (2, 1024, 1024, 2048): 2.43e-7, (1, 3000, 2048, 2048): 2.06e-7, (2, 2049, 2048, 4096): 2.37e-7,
    (2, 10, 16, 32): 1.67e-7, (2, 16, 16, 16): 1.64e-7, (2, 17, 16, 48): 1.35e-7, (64, 40, 16, 32): 2.45e-7, (2, 80, 16, 48): 2.43e-7,
}


def sofa_run(shape, make, blocks=None):
    """The run both the restatement and the device are measured on: seeded filters with onset delays, `blocks` blocks of noise (at
    least 2K sub-blocks), one filter replaced half way. `make(channels, L, P, B)` returns an object with set_filter and
    process_block. Returns (worst error against oracle.SofaRenderer, scale)."""
    from oracle import oracle as O
    C, L, P, B = shape
    K = -(-L // P)
    if blocks is None:
        blocks = max(5, -(-2 * K // (B // P)))
    rng = np.random.default_rng(C * 1000 + L + P)
    flt = sofa_filters(rng, C, L)
    ref, dut = O.SofaRenderer(C, L, B), make(C, L, P, B)
    for c, (l, r) in enumerate(flt):
        d = (c % 3, (2 * c) % 5)
        dut.set_filter(c, l, r, *d)
        ref.set_filter(c, l, r, *d)
    gains = (0.5 + 0.5 * rng.random(C)).astype(np.float32)
    worst = scale = 0.0
    for blk in range(blocks):
        x = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
        if blk == blocks // 2:
            l2, r2 = sofa_filters(rng, 1, L)[0]
            dut.set_filter(C - 1, l2, r2, 0, 1)
            ref.set_filter(C - 1, l2, r2, 0, 1)
        got, exp = dut.process_block(x, gains), ref.process_block(x, gains)
        worst = max(worst, float(np.abs(got.astype(np.float64) - exp).max()))
        scale = max(scale, float(np.abs(exp).max()))
    return worst, max(1.0, scale)


# ---------------------------------------------------------------- hrtfrender: which form serves; taps of one static direction

def hrtf_expected_transform(length, block, method):
    """the overlap-save transform: the next power of two holding length - 1 + block, served for 512 .. 4096 points; method 1 pins
    it where it fits, method 2 pins the FIR (0), method 0 takes it from 384 taps on"""
    n = 1 << max(length - 1 + block - 1, 0).bit_length()
    fits = 512 <= n <= 4096
    if method == 2 or not fits or (method == 0 and length < 384):
        return 0
    return n


def hrir_taps(sphere_bytes, face, uvw):
    """the barycentric blend of the three HRIR pairs of `face`: (left[len], right[len]) in f64"""
    import struct
    magic, _rate, flen, nv, ni = struct.unpack_from("<4s4I", sphere_bytes, 0)
    assert magic == b"HRIR"
    idx = np.frombuffer(sphere_bytes, "<u4", ni, 20)
    base = 20 + 4 * ni
    stride = 12 + 8 * flen
    ears = []
    for e in range(2):
        t = np.zeros(flen)
        for k in range(3):
            v = int(idx[3 * face + k])
            h = np.frombuffer(sphere_bytes, "<f4", flen, base + v * stride + 12 + 4 * flen * e).astype(np.float64)
            t += h * float(uvw[k])
        ears.append(t)
    return ears[0], ears[1]
