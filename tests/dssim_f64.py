"""tests/dssim_f64.py - the yardstick of the Dssim fast form: oracle/dssim_restate.py evaluated in f64. TEST INFRASTRUCTURE ONLY.

`load("f64")` loads a SECOND instance of the restatement's own text under another module name and switches its number
format: F = np.float64, and KERNEL / D65 / EPSILON / K rebuilt from their decimal constants in f64. Nothing of the algorithm
is restated here. `load("sep")` is that f64 instance with one substitution, the one that defines the fast form:
every 3x3 pass becomes a horizontal then a vertical 3-tap pass with the gain-matched taps
[0.30876, 0.38248, 0.30876] * sqrt(1.000001), each pass replicating its own edges. `load("sep5")` merges the two passes of
a blur into one 5-tap pass per axis over a SYMMETRICALLY padded line (edge sample included in the mirror), which is the
same function as two replicated 3-tap passes - the form the device kernel evaluates.

The case generator is deterministic: four contents x four amplitudes per size, seeded by w * h + amplitude, 20 % translucent
pixels where the frame is RGBA.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTATE = os.path.join(ROOT, "oracle", "dssim_restate.py")

TAP_GAIN = 1.000001           # sum of the published 3x3 weights
TAPS_1D = np.array([0.30876, 0.38248, 0.30876], np.float64) * np.sqrt(TAP_GAIN)
CONTENTS = ("gradient", "noise", "nearblack", "flat200")
AMPLITUDES = (1, 8, 40, 255)  # 255: an unrelated frame
_loaded = {}


def _pass_1d(p, axis):
    q = np.pad(p, [(1, 1) if a == axis else (0, 0) for a in range(2)], mode="edge")
    n = p.shape[axis]
    sl = lambda k: tuple(slice(k, k + n) if a == axis else slice(None) for a in range(2))
    return (q[sl(0)] * TAPS_1D[0] + q[sl(1)] * TAPS_1D[1]) + q[sl(2)] * TAPS_1D[2]


def _sep_blur_pass(p):
    return _pass_1d(_pass_1d(p, 1), 0)


def _merged_1d(p, axis):
    a, b = TAPS_1D[0], TAPS_1D[1]
    taps = (a * a, 2 * a * b, 2 * a * a + b * b, 2 * a * b, a * a)
    n = p.shape[axis]
    idx = np.arange(-2, n + 2)
    idx = np.where(idx < 0, -1 - idx, np.where(idx >= n, 2 * n - 1 - idx, idx)).clip(0, n - 1)   # symmetric padding
    q = np.take(p, idx, axis=axis)
    sl = lambda k: tuple(slice(k, k + n) if ax == axis else slice(None) for ax in range(2))
    acc = 0.0
    for k in range(5):
        acc = acc + q[sl(k)] * taps[k]
    return acc


def load(kind):
    """kind: "f32" (the restatement as it is), "f64", "sep" (f64, separable gain-matched passes), "sep5" (f64, merged 5-tap)."""
    if kind in _loaded:
        return _loaded[kind]
    spec = importlib.util.spec_from_file_location("dssim_restate_" + kind, RESTATE)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    if kind != "f32":
        F = m.F = np.float64
        m.KERNEL = np.array([0.095332, 0.118095, 0.095332, 0.118095, 0.146293, 0.118095, 0.095332, 0.118095, 0.095332], F)
        m.D65 = (F(0.9505), F(1.0), F(1.089))
        m.EPSILON = F(216.0) / F(24389.0)
        m.K = F(24389.0) / (F(27.0) * F(116.0))
    if kind == "sep":
        m.blur_pass = _sep_blur_pass
    elif kind == "sep5":
        m.blur = lambda p: _merged_1d(_merged_1d(p, 1), 0)
    elif kind not in ("f32", "f64"):
        raise ValueError(kind)
    _loaded[kind] = m
    return m


def _content(name, w, h, rng):
    y, x = np.mgrid[0:h, 0:w]
    if name == "gradient":
        px = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1)
    elif name == "noise":
        px = rng.integers(0, 256, (h, w, 3))
    elif name == "nearblack":
        px = rng.integers(0, 6, (h, w, 3))
    else:
        px = np.full((h, w, 3), 200)
    return px.astype(np.int64)


def make_case(w, h, channels, content, amp, stride=None):
    """-> (ref, mod, stride): two packed u8 frames (rows padded to `stride` with 0xA5 bytes)."""
    rng = np.random.default_rng(w * h + amp)
    ref = _content(content, w, h, rng)
    if amp == 255:
        mod = rng.integers(0, 256, (h, w, 3)).astype(np.int64)
    else:
        mod = np.clip(ref + rng.integers(-amp, amp + 1, (h, w, 3)), 0, 255)
    frames = []
    for px in (ref, mod):
        if channels == 4:
            alpha = np.where(rng.random((h, w)) < 0.2, rng.integers(0, 255, (h, w)), 255)
            px = np.concatenate([px, alpha[..., None]], -1)
        row = w * channels
        st = stride or row
        buf = np.full((h, st), 0xA5, np.uint8)
        buf[:, :row] = px.astype(np.uint8).reshape(h, row)
        frames.append(buf.reshape(-1))
    return frames[0], frames[1], stride or w * channels


def suite(w, h, channels=None, stride=None):
    """The 16 cases of a size: (name, ref, mod, stride, channels). channels None: RGB and RGBA alternate over the suite."""
    out = []
    for ci, content in enumerate(CONTENTS):
        for ai, amp in enumerate(AMPLITUDES):
            ch = channels or (4 if (ci + ai) % 2 else 3)
            ref, mod, st = make_case(w, h, ch, content, amp, stride)
            out.append(("%s-%d-%dch" % (content, amp, ch), ref, mod, st, ch))
    return out


def evaluate(kind, ref, mod, w, h, stride, channels, pattern=True):
    """-> (dssim value, [SSIM map per scale]) of one pair under `kind`."""
    m = load(kind)
    a = m.DssimImage(ref, w, h, stride, channels, pattern)
    b = m.DssimImage(mod, w, h, stride, channels, pattern)
    d, maps = m.compare(a, b, return_maps=True)
    return float(d), [np.asarray(x, np.float64) for x in maps]


def noise(cases, w, h, pattern=True):
    """f32 rounding noise of the exact form over `cases`: (N_d, N_map, [(d64, maps64) per case])."""
    n_d = n_map = 0.0
    ref64 = []
    for _, ref, mod, st, ch in cases:
        d32, m32 = evaluate("f32", ref, mod, w, h, st, ch, pattern)
        d64, m64 = evaluate("f64", ref, mod, w, h, st, ch, pattern)
        n_d = max(n_d, abs(d32 - d64))
        n_map = max(n_map, max(float(np.abs(x - y).max()) for x, y in zip(m32, m64)))
        ref64.append((d64, m64))
    return n_d, n_map, ref64
