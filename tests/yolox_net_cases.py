"""Seeded cases of yoloxinference's network for tests/test_yolox_net_cpu.py and tests/test_gpu_yolox_net.py: parameter
sets, u8 noise frames and the restatement's references (tests/yolox_net_restate.py), each computed once and shared.

Parameters: conv weights ~ N(0, 1.5^2 / fan_in), BatchNorm gamma in [0.8, 1.2], beta in [-0.2, 0.2], running mean in [-0.2, 0.2],
running var in [0.5, 1.5], prediction biases in [-1, 1]. Every set passes its builder's guards, computed here on the CPU with the
restatement alone (_guarded_references): in f64 every raw map finite with a standard deviation of at least 0.05 and every intermediate
activation with a nonzero spread - a degenerate net that outputs its biases would pass any tolerance - and a whole-net yardstick that
is not below f32's own resolution. A seeded set that misses a guard gives way to the next seed; the guards stay."""
import functools

import numpy as np

import yolox_net_restate as R

# name -> (depth, width, depthwise)
CONFIGS = {
    "nano": (0.33, 0.25, True),
    "tiny": (0.33, 0.375, False),          # channel counts 24, 48, 96 ..: no multiple of a tile
    "s_width": (0.33, 0.5, False),
    "deep_c3": (0.67, 0.25, False),        # two-deep C3 blocks with shortcuts
    "nano_dense": (0.33, 0.25, False),     # nano's shapes without depthwise
}
CLASSES = (1, 3)
SHAPES = ((32, 32), (64, 96))              # (H, W): levels 4x4, 2x2, 1x1; and a non-square one
N_FRAMES = (1, 3)
SEED = 20240

STOCK = {"nano": (0.33, 0.25, True), "tiny": (0.33, 0.375, False), "s": (0.33, 0.50, False), "m": (0.67, 0.75, False), "l": (1.0, 1.0, False),
         "x": (1.33, 1.25, False)}         # yolox.rs:40-222


@functools.lru_cache(maxsize=None)
def model(config, num_classes):
    return R.Yolox(*CONFIGS[config], num_classes)


def seeded_params(net, seed):
    rng = np.random.default_rng(seed)
    P = {}
    for name, shape in net.params:
        if name.endswith(".bn.weight"):
            a = rng.uniform(0.8, 1.2, shape)
        elif name.endswith(".bn.bias") or name.endswith(".bn.running_mean"):
            a = rng.uniform(-0.2, 0.2, shape)
        elif name.endswith(".bn.running_var"):
            a = rng.uniform(0.5, 1.5, shape)
        elif name.endswith(".bias"):
            a = rng.uniform(-1.0, 1.0, shape)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            a = rng.normal(0.0, 1.5 / np.sqrt(fan_in), shape)
        P[name] = a.astype(np.float32)
    return P


class GuardMiss(Exception):
    """a seeded set misses a guard of its case builder: the next seed is taken"""


MAPS = (("reg", slice(0, 4)), ("obj", slice(4, 5)), ("cls", slice(5, None)))   # the three raw maps of a level, as rows of [5 + C, h, w]
U = 2.0 ** -24


def _guarded_references(net, P, num_classes, H, W):
    """The f64 and f32 restatement of the three frames of a shape; GuardMiss unless, in f64, every raw map is finite with a standard
    deviation of at least 0.05 and every intermediate activation has a nonzero spread, and, for every n_frames of the cases, the f32
    restatement's max-abs error of every map - the whole-net test's yardstick - is at least u max|map|, u = 2^-24. (That is the bound of
    ONE f32 rounding of the map's largest value. A yardstick below it says the f32 restatement landed on the rounded f64 value by
    chance - it happens where a map is a single value - and measures no f32 noise; no f32 result but the correctly rounded one
    could then be within a multiple of it.)"""
    x = R.input_tensor(frames(H, W, 3))
    taps = {}
    m64, m32 = net.forward(P, x, np.float64, taps), net.forward(P, x, np.float32)
    for l, m in enumerate(m64):
        assert m.shape == (3, 5 + num_classes, H >> (3 + l), W >> (3 + l))
        for f in range(3):
            for what, rows in MAPS:
                part = m[f, rows]
                spread = part if part.size > 1 else m[:, rows]   # a map of ONE value (1 x 1 level, one channel): across the three frames
                if not (np.isfinite(part).all() and spread.std() >= 0.05):
                    raise GuardMiss((l, f, what))
        for n in N_FRAMES:
            for what, rows in MAPS:
                yard = np.abs(m32[l][:n, rows].astype(np.float64) - m[:n, rows]).max()
                if not yard >= U * np.abs(m[:n, rows]).max():
                    raise GuardMiss((l, n, what, "yardstick below one f32 rounding"))
    for name, act in taps.items():
        if not (np.isfinite(act).all() and act.max() > act.min()):
            raise GuardMiss(name)
    for m in m64 + m32:
        m.setflags(write=False)
    return {"float64": m64, "float32": m32}


@functools.lru_cache(maxsize=None)
def _seeded_set(config, num_classes):
    """(parameters, {(H, W): references}) of the first seed whose set passes the guards at every shape"""
    net = model(config, num_classes)
    first = SEED + 97 * list(CONFIGS).index(config) + num_classes
    for k in range(32):
        P = seeded_params(net, first + 1000 * k)
        try:
            return P, {(H, W): _guarded_references(net, P, num_classes, H, W) for (H, W) in SHAPES}
        except GuardMiss:
            continue
    raise AssertionError("no seed passes the guards")


def params(config, num_classes):
    return _seeded_set(config, num_classes)[0]


@functools.lru_cache(maxsize=None)
def frames(H, W, n_frames=3):
    """[n, H, W, 3] u8 noise; the first frames of a larger batch are those of a smaller one"""
    return np.random.default_rng(SEED + H * 7 + W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)[:n_frames]


class Case:
    def __init__(self, config, num_classes, H, W, n_frames):
        self.config, self.C, self.H, self.W, self.n = config, num_classes, H, W, n_frames
        self.name = "%s-c%d-%dx%d-n%d" % (config, num_classes, H, W, n_frames)
        self.net = model(config, num_classes)
        self.frames = frames(H, W, n_frames)

    @property
    def P(self):
        return params(self.config, self.C)

    def cfg(self):
        import mi355fx
        return mi355fx.yolox_net_config(*CONFIGS[self.config], self.C)

    def ref(self, dtype):
        """per level [n, 5 + C, h, w] of the restatement in `dtype`. A batch of one is the first frame of the batch of three."""
        full = _reference(self.config, self.C, self.H, self.W, np.dtype(dtype).name)
        return [m[:self.n] for m in full]


def _reference(config, num_classes, H, W, dtype_name):
    return _seeded_set(config, num_classes)[1][(H, W)][dtype_name]


def all_cases():
    return [Case(c, k, H, W, n) for c in CONFIGS for k in CLASSES for (H, W) in SHAPES for n in N_FRAMES]


# ---- the compositions (frames -> decoded tensor / detections): the seeded sets give raw maps in the thousands (u8 input, gain above
# one per layer), where every sigmoid is 0 or 1 and every exp overflows. For these tests the nine prediction layers' weights are
# rescaled per layer so that each raw map has a spread of about 2 around its bias; everything else is the seeded set.

@functools.lru_cache(maxsize=None)
def composition_params(config, num_classes, H=64, W=96):
    P = dict(params(config, num_classes))
    maps = _reference(config, num_classes, H, W, "float64")
    for l, m in enumerate(maps):
        for branch, rows in (("reg", slice(0, 4)), ("obj", slice(4, 5)), ("cls", slice(5, None))):
            name = "head.%s_preds.%d" % (branch, l)
            centred = m[:, rows] - P[name + ".bias"].astype(np.float64).reshape(1, -1, 1, 1)
            P[name + ".weight"] = (P[name + ".weight"].astype(np.float64) * (2.0 / centred.std())).astype(np.float32)
    return P


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def gap_threshold(values, lo_frac, hi_frac, min_gap):
    """A threshold in the widest gap between neighbours of sorted(values) with between lo_frac and hi_frac of the values ABOVE it; the
    midpoint guard: no value within min_gap / 2 of it, so f32 noise in the maps moves no candidate across."""
    s = np.sort(np.asarray(values, np.float64).reshape(-1))
    n = len(s)
    lo, hi = max(int(np.ceil(n * (1 - hi_frac))), 1), min(int(np.floor(n * (1 - lo_frac))), n - 1)
    ks = np.arange(lo, hi + 1)
    assert len(ks) > 0
    k = ks[np.argmax(s[ks] - s[ks - 1])]
    assert s[k] - s[k - 1] >= min_gap, (s[k] - s[k - 1], min_gap)
    return float((s[k] + s[k - 1]) / 2), int(n - k)


class CompositionCase(Case):
    """A case with the rescaled prediction layers and thresholds chosen from its f64 maps."""

    @property
    def P(self):
        return composition_params(self.config, self.C, self.H, self.W)

    def __init__(self, config, num_classes, H, W, n_frames):
        super().__init__(config, num_classes, H, W, n_frames)
        self.maps64 = self.net.forward(self.P, R.input_tensor(self.frames), np.float64)
        for m in self.maps64:
            assert np.isfinite(m).all() and np.abs(m).max() < 40.0 and m.std() > 0.25, (np.abs(m).max(), m.std())   # exp and sigmoid stay in range
        self.A = sum(m.shape[2] * m.shape[3] for m in self.maps64)
        obj = np.concatenate([sigmoid64(m[:, 4]).reshape(self.n, -1) for m in self.maps64], axis=1)          # [n, A]
        cls = np.concatenate([sigmoid64(m[:, 5:]).max(axis=1).reshape(self.n, -1) for m in self.maps64], axis=1)
        # f32 noise: the whole-net test holds the maps to a few 1e-6 of their magnitude; a sigmoid moves by at most a quarter of that
        self.box_thr, _ = gap_threshold(obj, 0.15, 0.45, 1e-4)
        stay = obj >= self.box_thr
        self.cls_thr, _ = gap_threshold(cls[stay], 0.5, 0.9, 1e-4)
        self.survivors = [int((stay[f] & (cls[f] >= self.cls_thr)).sum()) for f in range(self.n)]
        assert all(1 <= s <= self.A // 2 for s in self.survivors), (self.survivors, self.A)
        self.params = (np.float32(self.box_thr), np.float32(self.cls_thr), np.float32(0.45))
