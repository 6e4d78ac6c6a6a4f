"""Independent restatement of agingradio (AgingRadio::process, audio/audiofx/src/agingradio/imp.rs:94-136) as DESIGN §4.9 states
it: the lowpass-filter 0.4.1 single-pole filter (parity unpinned) and the Philox4x32-10 draws that replace rand::rng(). Plain Python
+ numpy in IEEE f64 with nothing fused: the device must agree bit for bit. Used by tests/test_agingradio_cpu.py and
tests/test_gpu_agingradio.py; not part of the product."""
import math

import numpy as np

M32 = 0xFFFFFFFF
ALWAYS = (1 << 64) - 1   # Bernoulli's p_int for p == 1

DEFAULTS = dict(white_noise_ampl=0.011, clicks_prob=1.0 / 100000.0, lowpass_freq=2000, bits_to_quantize=4.0,
                cubic_curve_distortion=1.0, cubic_curve_passes=3)   # imp.rs:51-56
OFF = dict(white_noise_ampl=0.0, clicks_prob=0.0, lowpass_freq=0, bits_to_quantize=0.0, cubic_curve_distortion=0.0, cubic_curve_passes=0)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & np.uint64(M32) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    m0, m1, w0, w1, mask, sh = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return c0, c1, c2, c3


def draws(pairs, j, seed):
    """draw j of every frame pair in `pairs`: 64-bit word j & 1 of Philox(counter (pair_lo, pair_hi, j >> 1, 0), key seed)."""
    pairs = np.asarray(pairs, np.uint64)
    x0, x1, x2, x3 = philox4x32_10(pairs & np.uint64(M32), pairs >> np.uint64(32), np.full(pairs.shape, j >> 1, np.uint64), np.zeros(pairs.shape, np.uint64),
                                   seed & M32, seed >> 32)
    lo, hi = (x0, x1) if j % 2 == 0 else (x2, x3)
    return (hi << np.uint64(32)) | lo


def p_int(p):
    """rand 0.9 Bernoulli::new(p): p == 1 always, else (p * 2^64) as u64."""
    p = float(np.float32(p))
    return ALWAYS if p >= 1.0 else int(p * 18446744073709551616.0)


def noise(u, a):
    """rand 0.9 UniformFloat::sample_single(-a, a): value1_2 from the top 52 bits, minus 1, times (high - low), plus low."""
    v = ((u >> np.uint64(12)) | np.uint64(0x3FF0000000000000)).view(np.float64) - 1.0
    scale = a + a
    t = v * scale
    return t + (-a)


def lowpass_alpha(rate, cutoff):
    """LowpassFilter::<f64>::new(rate, cutoff) (lowpass-filter 0.4.1)."""
    rc = 1.0 / (float(cutoff) * 2.0 * math.pi)
    dt = 1.0 / float(rate)
    return dt / (rc + dt)


def round_half_away(x):
    t = np.trunc(x)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x - t) >= 0.5, t + np.sign(x), t)


class AgingRadio:
    """One instance: setup (imp.rs:326-345) then process per buffer. `k` counts the frame pairs processed since setup."""

    def __init__(self, channels, rate, lowpass_freq, seed):
        self.channels, self.seed, self.k = channels, seed, 0
        self.alpha = lowpass_alpha(rate, lowpass_freq) if lowpass_freq > 0 else None
        self.y = np.zeros(channels) if lowpass_freq > 0 else None

    def process(self, data, white_noise_ampl, clicks_prob, bits_to_quantize, cubic_curve_distortion, cubic_curve_passes, **_):
        """data: interleaved f32 / f64 samples (frames * channels). Returns the processed copy."""
        ch = self.channels
        out = np.array(data, copy=True)
        P = out.size // ch // 2
        if P == 0:
            return out
        pairs = np.arange(P, dtype=np.uint64) + np.uint64(self.k)
        x = out[: P * 2 * ch].astype(np.float64).reshape(P, 2 * ch)
        p = float(np.float32(clicks_prob))
        if p > 0:
            pi = p_int(p)
            click = np.ones(P, bool) if pi == ALWAYS else draws(pairs, 0, self.seed) < np.uint64(pi)
        else:
            click = np.zeros(P, bool)
        a = float(np.float32(white_noise_ampl))
        if a > 0:
            for c in range(2 * ch):
                n = noise(draws(pairs, 1 + c, self.seed), a)
                assert np.all(n < a) and np.all(n >= -a)
                x[:, c] = x[:, c] + n
        if self.alpha is not None:
            x = np.where(x < -1.0, -1.0, np.where(x > 1.0, 1.0, x))   # f64::clamp: NaN stays NaN
            y, al = self.y, self.alpha
            with np.errstate(invalid="ignore", over="ignore"):
                for q in np.flatnonzero(~click):
                    row = x[q]
                    y = y + al * (row[:ch] - y)
                    row[:ch] = y
                    y = y + al * (row[ch:] - y)
                    row[ch:] = y
            self.y = y
        b = float(np.float32(bits_to_quantize))
        with np.errstate(invalid="ignore", over="ignore"):
            if b > 0:
                f = math.pow(2.0, b)
                x = round_half_away(x * f) / f
            d = float(np.float32(cubic_curve_distortion))
            if d > 0 and cubic_curve_passes > 0:
                for _ in range(int(cubic_curve_passes)):
                    x = x - d * (x * (x * x))
        x[click] = 1.0
        with np.errstate(over="ignore"):
            out[: P * 2 * ch] = x.reshape(-1).astype(out.dtype)
        self.k += P
        return out
