"""Case builders for the YOLOX head decoder, shared by tests/test_yolox_head_cpu.py and tests/test_gpu_yolox_head.py.
Everything is seeded and small. A Head holds the level maps of one tensor - (reg, obj, cls, stride) per level - one settings triple
and, for the truncation case, an output capacity; tensor() and expected() are the numpy restatement's answers
(tests/yolox_head_restate.py), computed once. Every builder asserts that no f64 value behind the stated deviation lies within 16 f64
ULP of an f32 rounding midpoint (handdec_restate.near_tie): the cases hold for any f64 libm that good. A seed that trips the guard is
replaced by the next one; nothing is skipped or masked."""
import numpy as np

import yolox_head_restate as R
from handdec_restate import near_tie

F32 = np.float32
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]

# the level sets of the shape tests; (15, 17), (1, 2): A = 257 with the level boundary at 255, inside a wave and next to a tile edge
LEVEL_SETS = {
    "one": [(1, 1)],
    "row65": [(1, 65)],
    "three_small": [(3, 5), (2, 3), (1, 1)],
    "boundary255": [(15, 17), (1, 2)],
    "three_square": [(16, 16), (8, 8), (4, 4)],
    "eight": [(2, 3)] * 8,
}
CLASSES = (1, 2, 80, 128)
STRIDES = (8, 16, 32, 7, 1, 3, 64, 5)


class Head:
    def __init__(self, name, levels, params, max_dets=None):
        self.name = name
        self.levels = [(np.ascontiguousarray(r, np.float32), np.ascontiguousarray(o, np.float32), np.ascontiguousarray(c, np.float32), int(s))
                       for r, o, c, s in levels]
        for r, o, c, _ in self.levels:
            assert r.shape[0] == 4 and o.shape == (1,) + r.shape[1:] and c.shape[1:] == r.shape[1:]
        self.params = tuple(float(F32(v)) for v in params)
        self.max_dets = max_dets
        self._tensor = self._expected = None
        assert not near_tie(R.deviation64(self.levels)).any(), name

    @property
    def C(self):
        return self.levels[0][2].shape[0]

    @property
    def A(self):
        return sum(r.shape[1] * r.shape[2] for r, _, _, _ in self.levels)

    def tensor(self):
        if self._tensor is None:
            self._tensor = R.tensor(self.levels)
            self._tensor.setflags(write=False)
        return self._tensor

    def expected(self):
        """The full (untruncated) answer."""
        if self._expected is None:
            self._expected = R.dets(self.levels, *self.params, decoded=self.tensor())
            self._expected.setflags(write=False)
        return self._expected

    def __repr__(self):
        return "Head(%s)" % self.name


def random_levels(seed, shapes, strides, n_classes, obj_shift=0.0):
    """Offsets within a cell or two, sizes of a few cells (neighbours overlap: NMS has work), logits normal(0, 4)."""
    rng = np.random.default_rng(seed)
    levels = []
    for (h, w), s in zip(shapes, strides):
        reg = np.concatenate([rng.normal(0.0, 2.0, (2, h, w)), rng.normal(1.0, 0.5, (2, h, w))]).astype(np.float32)
        obj = (rng.normal(0.0, 4.0, (1, h, w)) + obj_shift).astype(np.float32)
        cls = rng.normal(0.0, 4.0, (n_classes, h, w)).astype(np.float32)
        levels.append((reg, obj, cls, s))
    return levels


def guarded(seed, make):
    """make(seed) -> levels; the first seed from `seed` on whose levels pass the midpoint guard."""
    for k in range(1000):
        levels = make(seed + k)
        if not near_tie(R.deviation64(levels)).any():
            return levels
    raise AssertionError("no seed passes the guard")


def random_head(name, seed, shapes, strides, n_classes, params=(0.5, 0.5, 0.45), max_dets=None, obj_shift=0.0):
    return Head(name, guarded(seed, lambda s: random_levels(s, shapes, strides, n_classes, obj_shift)), params, max_dets)


_cache = {}


def shape_head(set_name, n_classes):
    key = (set_name, n_classes)
    if key not in _cache:
        shapes = LEVEL_SETS[set_name]
        seed = 1000 * (list(LEVEL_SETS).index(set_name) + 1) + n_classes
        _cache[key] = random_head("shape_%s_C%d" % key, seed, shapes, STRIDES[:len(shapes)], n_classes)
    return _cache[key]


# ---------------------------------------------------------------- known answers by hand

def kat_head():
    """One candidate of interest per level of a three-level head with non-square levels: level 0 (2 x 3, stride 8) element (y 1, x 2),
    level 1 (3 x 2, stride 16) element (y 2, x 1), level 2 (1 x 2, stride 32) element (y 0, x 1). Everything else has obj = -110."""
    shapes, strides = [(2, 3), (3, 2), (1, 2)], (8, 16, 32)
    picks = [(1, 2), (2, 1), (0, 1)]
    levels = []
    for (h, w), s, (y, x) in zip(shapes, strides, picks):
        reg = np.zeros((4, h, w), np.float32)
        obj = np.full((1, h, w), -110.0, np.float32)
        cls = np.full((2, h, w), -110.0, np.float32)
        reg[:, y, x] = (0.5, 0.25, 0.0, 0.0)      # cx = (0.5 + x) * s, cy = (0.25 + y) * s, w = h = exp(0) * s = s
        obj[0, y, x] = 20.0                        # sigmoid -> 1
        cls[1, y, x] = 0.0                         # sigmoid -> 0.5, class 1
        levels.append((reg, obj, cls, s))
    head = Head("kat", levels, (0.5, 0.25, 0.5))
    # candidate = level start + y * w + x; (cx, cy, w, h)
    rows = [(0 + 1 * 3 + 2, (20.0, 10.0, 8.0, 8.0)), (6 + 2 * 2 + 1, (24.0, 36.0, 16.0, 16.0)), (12 + 0 * 2 + 1, (48.0, 8.0, 32.0, 32.0))]
    return head, rows


# ---------------------------------------------------------------- the class-tie property

def sigmoid_run(min_len=4):
    """Adjacent f32 logits, descending, that share ONE f32 sigmoid and pass the guard."""
    for start in (5.0, 5.125, 5.25, 5.5, 6.0, 6.5):
        top = F32(start)
        # walk down from `top` to the first logit whose sigmoid changes: a whole run of one sigmoid value lies below it
        x = top
        while R.sigmoid32(x) == R.sigmoid32(top):
            x = np.nextafter(x, F32(-np.inf))
        run, v = [], R.sigmoid32(x)
        while R.sigmoid32(x) == v:
            run.append(x)
            x = np.nextafter(x, F32(-np.inf))
        run = np.array(run, np.float32)
        if len(run) >= min_len and not near_tie(R.sigmoid64(run)).any():
            return run
    raise AssertionError("no run passes the guard")


def tie_head():
    """One level (1, 5), one candidate per rule; obj = 20 (sigmoid 1), boxes far apart. Returns (head, class per candidate)."""
    run = sigmoid_run()
    n_classes = max(len(run), 3) + 2
    rows = [
        ([-20.0] + list(run) + [-20.0] * (n_classes - 1 - len(run)), len(run)),     # the run, descending: its last index wins
        ([20.0, 30.0, 25.0] + [-3.0] * (n_classes - 3), 2),                         # all three saturate to 1: the last
        ([-110.0] * n_classes, n_classes - 1),                                      # all 0: class C - 1
        ([-120.0, -111.0] + [-110.0] * (n_classes - 3) + [-5.0], n_classes - 1),    # a strict maximum at the end
        ([25.0] + [17.0] * (n_classes - 1), 0),                                     # 17 is below the saturation: class 0 alone is 1
    ]
    w = len(rows)
    reg = np.zeros((4, 1, w), np.float32)
    obj = np.full((1, 1, w), 20.0, np.float32)
    cls = np.array([r[0] for r in rows], np.float32).T.reshape(n_classes, 1, w)
    return Head("ties", [(reg, obj, cls, 64)], (0.5, 0.0, 0.5)), [r[1] for r in rows]


# ---------------------------------------------------------------- the unfused add and multiply

def unfused_head():
    """Strides that are no power of two: (reg + g) * s rounds twice. The case has discriminating power only if ONE rounding would have
    given another answer for many candidates; asserted here."""
    head = random_head("unfused", 77, [(15, 17), (1, 2)], (7, 13), 3)
    t, f = head.tensor()[:, :2], R.fused_xy(head.levels)
    differs = (t.view(np.uint32) != f.view(np.uint32)).any(axis=1)
    assert differs.mean() >= 0.25, differs.mean()
    return head


# ---------------------------------------------------------------- objectness drop, non-finite values

def objdrop_head():
    """Classes all 1.0. obj just below the threshold 0.5 (dropped), just above (kept), NaN (kept: NaN < thr is false)."""
    w = 6
    reg = np.zeros((4, 1, w), np.float32)
    obj = np.array([-1e-6, 1e-6, QNAN, -1e-6, 1e-6, -30.0], np.float32).reshape(1, 1, w)
    cls = np.full((3, 1, w), 30.0, np.float32)
    cls[1:, 0, 2] = -30.0      # the NaN candidate alone in class 0: the sign of its NaN confidence (the hardware's) orders nothing
    head = Head("objdrop", [(reg, obj, cls, 64)], (0.5, 0.5, 0.5))
    return head, [1, 2, 4]


def nonfinite_head():
    """reg2 = 88.8: exp overflows to inf, the box is (-inf, inf) and the casts saturate; reg0 = NaN; reg3 = -110: a height of 0;
    obj = -95 and a class at -95: subnormal sigmoids and confidences; +-inf logits."""
    w = 8
    reg = np.zeros((4, 1, w), np.float32)
    reg[2, 0, 0] = 88.8
    reg[0, 0, 1] = QNAN
    reg[3, 0, 2] = -110.0
    reg[2, 0, 3] = np.inf
    reg[1, 0, 4] = -np.inf
    obj = np.full((1, 1, w), 20.0, np.float32)
    obj[0, 0, 5] = -95.0
    obj[0, 0, 6] = np.inf
    cls = np.full((2, 1, w), -2.0, np.float32)
    cls[1] = 3.0
    cls[:, 0, 4] = (-95.0, -np.inf)
    cls[:, 0, 5] = (-2.0, -np.inf)
    cls[:, 0, 7] = (np.inf, 17.0)
    return Head("nonfinite", [(reg, obj, cls, 32)], (0.0, 0.0, 0.5))


# ---------------------------------------------------------------- batches, sort path, truncation

def batch_heads(n, seed=300):
    """n heads of one shape with different content."""
    return [random_head("batch_%d" % k, seed + 50 * k, [(15, 17), (1, 2)], (8, 7), 9) for k in range(n)]


def batch_settings(k):
    rng = np.random.default_rng(40 + k)
    return (float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.3, 0.8)), float(rng.uniform(0.1, 0.8)))


def sort_head():
    """5376 candidates, all kept by thresholds of 0: above the 4096 keys that sort in LDS."""
    if "sort" not in _cache:
        _cache["sort"] = random_head("sort_global", 9100, [(64, 64), (32, 32), (16, 16)], (8, 16, 32), 2, params=(0.0, 0.0, 0.45))
    return _cache["sort"]


def trunc_head(cap):
    return random_head("trunc_%d" % cap, 5200, [(16, 16), (8, 8), (4, 4)], (8, 16, 32), 5, params=(0.4, 0.45, 0.45), max_dets=cap)


# ---------------------------------------------------------------- input frames

def frames(seed, n_frames, width, height, pad):
    """(bytes of n_frames frames at a pitch, frame_pitch, stride): rows padded by `pad` bytes of 0xEE, frames by 5 more."""
    rng = np.random.default_rng(seed)
    stride = 3 * width + pad
    pitch = stride * height + (5 if pad else 0)
    buf = np.full(n_frames * pitch, 0xEE, np.uint8)
    for f in range(n_frames):
        for y in range(height):
            at = f * pitch + y * stride
            buf[at: at + 3 * width] = rng.integers(0, 256, 3 * width, dtype=np.uint8)
    return buf, pitch, stride
