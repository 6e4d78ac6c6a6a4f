"""Case builders for the yolov8tensordec2 / yoloxtensordec decoder, shared by tests/test_yolodec_cpu.py and
tests/test_gpu_yolodec.py. Everything is seeded and small. A Case holds a tensor in its layout's shape ((F, N) for "V8", (N, F) for
"X"), one settings triple (box_thr, class_thr, iou_thr) and, for the truncation cases, an output capacity. expected() is the numpy
restatement's answer (tests/yolodec_restate.py), computed once per case."""
import numpy as np

import yolodec_restate as R

F32 = np.float32
QNAN_POS, QNAN_NEG = 0x7FC00000, 0xFFC00000


def bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


class Case:
    def __init__(self, name, layout, data, params, max_dets=None):
        self.name, self.layout = name, layout
        self.data = np.ascontiguousarray(data, dtype=np.float32)
        self.params = tuple(float(F32(v)) for v in params)
        self.max_dets = max_dets
        self._expected = None

    @property
    def F(self):
        return self.data.shape[0] if self.layout == "V8" else self.data.shape[1]

    @property
    def N(self):
        return self.data.shape[1] if self.layout == "V8" else self.data.shape[0]

    def expected(self):
        """The full (untruncated) answer."""
        if self._expected is None:
            self._expected = R.decode(self.data, self.layout, *self.params)
            self._expected.setflags(write=False)
        return self._expected

    def __repr__(self):
        return "Case(%s)" % self.name


def from_candidates(layout, cands, n_classes=None):
    """cands: rows of (x, y, w, h, [objectness for X], scores...) -> the tensor in its layout."""
    a = np.array(cands, np.float32)
    return np.ascontiguousarray(a.T) if layout == "V8" else a


# ---------------------------------------------------------------- the known-answer tensors, written out by hand

KAT_BOXES = [(4.5, 4.5, 9, 9, 0.9, 0.1),     # A: (0, 0)-(9, 9), class 0
             (4.5, 2.0, 9, 4, 0.8, 0.2),     # B: (0, 0)-(9, 4), class 0; IoU(A, B) = 50 / (100 + 50 - 50) = 0.5 exactly
             (100, 100, 9, 9, 0.3, 0.7)]     # C: (95.5, 95.5)-(104.5, 104.5), class 1
IOU_HALF_BELOW = float(np.nextafter(F32(0.5), F32(0)))
# (x, y, width, height, class, candidate)
KAT_A, KAT_B, KAT_C = (0, 0, 9, 9, 0, 0), (0, 0, 9, 4, 0, 1), (95, 95, 9, 9, 1, 2)


def kat_v8(iou_thr):
    return Case("kat_v8_%r" % iou_thr, "V8", from_candidates("V8", KAT_BOXES), (0.0, 0.4, iou_thr))


def kat_x(objectness, box_thr, iou_thr=0.5):
    rows = [b[:4] + (objectness,) + b[4:] for b in KAT_BOXES]
    return Case("kat_x_%r_%r_%r" % (objectness, box_thr, iou_thr), "X", from_candidates("X", rows), (box_thr, 0.4, iou_thr))


# name, case, expected (x, y, w, h, class, candidate) rows, expected confidences
def kats():
    c = [F32(0.9), F32(0.8), F32(0.7)]
    h = [F32(0.45), F32(0.4), F32(0.35)]
    return [
        (kat_v8(0.5), [KAT_A, KAT_B, KAT_C], c),                       # the strict `>`: IoU == threshold keeps B
        (kat_v8(IOU_HALF_BELOW), [KAT_A, KAT_C], [c[0], c[2]]),
        (kat_x(1.0, 0.25), [KAT_A, KAT_B, KAT_C], c),
        (kat_x(1.0, 0.25, IOU_HALF_BELOW), [KAT_A, KAT_C], [c[0], c[2]]),
        (kat_x(0.5, 0.25), [KAT_A, KAT_B, KAT_C], h),
        (kat_x(0.5, 0.6), [], []),
    ]


# ---------------------------------------------------------------- the argmax rule

def _spread(score_rows, layout, thr, name):
    """One candidate per score row, boxes far apart (NMS drops nothing)."""
    rows = []
    for k, s in enumerate(score_rows):
        head = (50.0 * k + 10, 20.0, 8, 6) + ((1.0,) if layout == "X" else ())
        rows.append(head + tuple(s))
    return Case(name, layout, from_candidates(layout, rows), (0.5, thr, 0.5))


# name -> (score rows, class threshold, expected class per candidate in tensor order), V8 and X unless noted
def argmax_cases():
    pz, nz, inf = F32(0.0), F32(-0.0), F32(np.inf)
    out = []
    for layout in ("V8", "X"):
        out += [
            (_spread([(0.5, 0.5, 0.5), (0.5, 0.5, 0.25), (0.25, 0.5, 0.5)], layout, 0.1, "equal_%s" % layout), [2, 1, 2]),
            (_spread([(pz, nz, nz), (nz, pz, nz), (nz, nz, pz), (nz, nz, nz)], layout, -1.0, "zeros_%s" % layout), [0, 1, 2, 2]),
            (_spread([(0.1, inf, 0.2), (inf, 0.3, inf)], layout, 0.5, "inf_%s" % layout), [1, 2]),
            (_spread([(-0.5, -0.25, -0.75), (-0.75, -0.5, -0.5)], layout, -1.0, "negative_%s" % layout), [1, 2]),
        ]
    # NaNs as INPUT values (V8: they pass through comparison and selection only)
    out += [
        # +NaN beats every number, is kept (NaN < thr is false) and sorts first in its class, before 0.99
        (_spread([(0.9, bits(QNAN_POS), 0.3), (0.1, 0.99, 0.2)], "V8", 0.5, "nan_pos_V8"), [1, 1]),
        # -NaN loses to every number
        (_spread([(-5.0, bits(QNAN_NEG), -7.0), (bits(QNAN_NEG), -3.0, -2.0)], "V8", -10.0, "nan_neg_V8"), [0, 2]),
    ]
    return out


# ---------------------------------------------------------------- ties

def tie_tensor():
    """Six candidates of one class with bit-equal confidence, each overlapping its neighbours: what is kept depends on the order."""
    rows = [(10.0 + 4 * k, 10.0, 10, 10, 0.75, 0.125) for k in range(6)]
    return from_candidates("V8", rows)


TIE_PERM = [3, 0, 5, 1, 4, 2]


def tie_cases():
    t = tie_tensor()
    return [Case("ties", "V8", t, (0.0, 0.5, 0.3)), Case("ties_permuted", "V8", t[:, TIE_PERM], (0.0, 0.5, 0.3))]


# ---------------------------------------------------------------- casts

def cast_case(layout="V8"):
    nan = bits(QNAN_POS)
    rows = [
        (3e9, 3e9, 10, 10),        # saturates upwards
        (-3e9, -3e9, 10, 10),      # saturates downwards
        (4.5, 9.25, 10, 19.5),     # xmin = -0.5 -> 0, ymin = -0.5 -> 0
        (200.0, 200.0, 0.99, 0.5), # width 0.99 -> 0
        (nan, 300.0, 10, 10),      # NaN x: xmin, xmax NaN -> x = width = 0; its IoU is NaN: it drops nothing and is not dropped
        (300.0, 300.0, 10, 10),    # shares y with the NaN box; kept
        (302.0, 300.0, 10, 10),    # dropped by the box before it, not by the NaN box
    ]
    confs = [0.9, 0.85, 0.8, 0.75, 0.95, 0.7, 0.65]
    full = [r + ((1.0,) if layout == "X" else ()) + (c, 0.0625) for r, c in zip(rows, confs)]
    return Case("casts_%s" % layout, layout, from_candidates(layout, full), (0.5, 0.5, 0.4))


# ---------------------------------------------------------------- synthetic tensors

def synth(seed, layout, F, N, frac=0.2, n_clusters=6, obj_lo=0.3, spread=6.0, n_hot_classes=None):
    """Low class scores everywhere, a share `frac` of the candidates with one confident class (one of the first n_hot_classes); boxes
    clustered so NMS has work."""
    rng = np.random.default_rng(seed)
    C = F - (4 if layout == "V8" else 5)
    scores = (rng.random((N, C), dtype=np.float32) * F32(0.3)).astype(np.float32)
    hot = rng.random(N) < frac
    hot_cls = rng.integers(0, min(C, n_hot_classes or C), N)
    scores[hot, hot_cls[hot]] = (F32(0.5) + rng.random(int(hot.sum()), dtype=np.float32) * F32(0.5)).astype(np.float32)
    centres = rng.random((n_clusters, 2), dtype=np.float32) * F32(600) + F32(20)
    which = rng.integers(0, n_clusters, N)
    xy = centres[which] + (rng.standard_normal((N, 2)) * spread).astype(np.float32)
    wh = (F32(30) + rng.random((N, 2), dtype=np.float32) * F32(30)).astype(np.float32)
    cols = [xy[:, 0], xy[:, 1], wh[:, 0], wh[:, 1]]
    if layout == "X":
        cols.append((F32(obj_lo) + rng.random(N, dtype=np.float32) * F32(1.0 - obj_lo)).astype(np.float32))
    a = np.concatenate([np.stack(cols, axis=1).astype(np.float32), scores], axis=1)
    assert a.shape == (N, F)
    return np.ascontiguousarray(a.T) if layout == "V8" else np.ascontiguousarray(a)


SHAPE_N = (1, 63, 64, 65, 255, 257, 1000)
SHAPE_F = (6, 7, 12, 84, 85, 133)


def shape_cases():
    out = []
    for layout in ("V8", "X"):
        for N in SHAPE_N:
            for F in SHAPE_F:
                out.append(Case("shape_%s_N%d_F%d" % (layout, N, F), layout, synth(N * 1000 + F, layout, F, N, frac=0.3), (0.5, 0.45, 0.45)))
    return out


def survivor_cases():
    out = []
    for layout in ("V8", "X"):
        t = synth(77, layout, 12, 300)
        out.append(Case("none_%s" % layout, layout, t, (0.5, 2.0, 0.45)))
        one = t.copy()
        if layout == "V8":
            one[4 + 3, 123] = 1.5
        else:
            one[123, 5 + 3] = 1.5
            one[123, 4] = 1.0
        out.append(Case("one_%s" % layout, layout, one, (0.5, 1.25, 0.45)))
        out.append(Case("all_%s" % layout, layout, t, (0.0, 0.0, 0.45)))
    return out


def grid_tensor(seed, layout, N, n_classes, single_class=False):
    """Every candidate survives a threshold of 0; boxes on a jittered grid so that NMS both keeps and drops."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(N)))
    k = np.arange(N)
    xy = np.stack([(k % side) * 12.0, (k // side) * 12.0], axis=1) + rng.uniform(-5, 5, (N, 2))
    wh = 10.0 + rng.uniform(-2, 6, (N, 2))
    scores = rng.random((N, n_classes), dtype=np.float32)
    if single_class:
        scores[:, 1:] *= F32(0.001)
        scores[:, 0] = F32(0.5) + scores[:, 0] * F32(0.5)
    cols = [xy.astype(np.float32), wh.astype(np.float32)]
    if layout == "X":
        cols.append((F32(0.5) + rng.random((N, 1), dtype=np.float32) * F32(0.5)).astype(np.float32))
    a = np.concatenate(cols + [scores], axis=1).astype(np.float32)
    return np.ascontiguousarray(a.T) if layout == "V8" else np.ascontiguousarray(a)


def sort_switch_cases():
    """4096 keys sort in LDS, 4097 in global scratch; 5000 of one class is one long run."""
    out = []
    for N in (4096, 4097):
        out.append(Case("grid_V8_N%d" % N, "V8", grid_tensor(N, "V8", N, 3), (0.0, 0.0, 0.3)))
        out.append(Case("grid_X_N%d" % N, "X", grid_tensor(N + 1, "X", N, 3), (0.0, 0.0, 0.3)))
    out.append(Case("grid_X_N5000_one_class", "X", grid_tensor(5000, "X", 5000, 1), (0.0, 0.0, 0.3)))
    out.append(Case("grid_V8_N5000_one_class", "V8", grid_tensor(5001, "V8", 5000, 2, single_class=True), (0.0, 0.0, 0.3)))
    return out


def truncation_cases():
    out = []
    for layout in ("V8", "X"):
        t = synth(5, layout, 10, 400, frac=0.5, n_clusters=40, spread=3.0)
        for cap in (0, 1, 7):
            out.append(Case("trunc_%s_%d" % (layout, cap), layout, t, (0.4, 0.45, 0.45), max_dets=cap))
    return out


def random_cases():
    out = []
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        layout = ("V8", "X")[seed % 2]
        C = int(rng.integers(1, 13))
        F = C + (4 if layout == "V8" else 5)
        if F < 6:
            F = 6
        N = int(rng.integers(1, 601))
        params = (float(rng.uniform(0.2, 0.7)), float(rng.uniform(0.2, 0.8)), float(rng.uniform(0.1, 0.8)))
        out.append(Case("random_%02d" % seed, layout, synth(2000 + seed, layout, F, N, frac=float(rng.uniform(0.05, 0.9)),
                                                            n_clusters=int(rng.integers(1, 10))), params))
    return out


def realistic(layout, seed=0):
    """The real shapes: V8 84 x 8400, X 8400 x 85, about 1 % of the candidates above threshold, clustered."""
    F = 84 if layout == "V8" else 85
    return Case("realistic_%s" % layout, layout, synth(9000 + seed, layout, F, 8400, frac=0.01 if layout == "V8" else 0.0125, n_clusters=12, obj_lo=0.2,
                      n_hot_classes=5),
                (0.36, 0.45, 0.45))


GROUPS = ("kat", "argmax", "ties", "casts", "shapes_V8", "shapes_X", "survivors", "sort_switch", "truncation", "random")
_cache = {}


def group(name):
    """The cases of one group; built once."""
    if name not in _cache:
        if name == "kat":
            c = [k[0] for k in kats()]
        elif name == "argmax":
            c = [a[0] for a in argmax_cases()]
        elif name == "ties":
            c = tie_cases()
        elif name == "casts":
            c = [cast_case("V8"), cast_case("X")]
        elif name in ("shapes_V8", "shapes_X"):
            c = [s for s in shape_cases() if s.layout == name[-2:].lstrip("_")]
        elif name == "survivors":
            c = survivor_cases()
        elif name == "sort_switch":
            c = sort_switch_cases()
        elif name == "truncation":
            c = truncation_cases()
        elif name == "random":
            c = random_cases()
        else:
            raise KeyError(name)
        _cache[name] = c
    return _cache[name]


def all_cases():
    return [c for g in GROUPS for c in group(g)]
