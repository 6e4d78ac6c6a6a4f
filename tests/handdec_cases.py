"""Case builders for the handdetectiontensordec / handlandmarktensordec decoders, shared by tests/test_handdec_cpu.py and
tests/test_gpu_handdec.py. Everything is seeded and small. A PalmCase holds a [N, 8] tensor and one params tuple (confidence_thr,
nms_iou_thr, max_hands, frame or None); a LandmarkCase a [H, 21 * D] tensor, an optional score vector and the same tuple. expected()
is the numpy restatement's answer (tests/handdec_restate.py), computed once per case. Every builder asserts that no f64 value
behind deviation a lies at an f32 rounding midpoint (R.near_tie): the cases hold for any f64 libm within 16 ULP."""
import numpy as np

import handdec_restate as R

F32 = np.float32
QNAN_POS, QNAN_NEG = 0x7FC00000, 0xFFC00000
FRAMES = (None, (192, 192), (640, 360))


def bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def _params(p):
    conf, iou, max_hands, frame = p
    return (float(F32(conf)), float(F32(iou)), int(max_hands), None if frame is None else (int(frame[0]), int(frame[1])))


def flat_params(p):
    """(conf, iou, max_hands, frame) -> the five values Context.handdec_* and the C++ restatement take."""
    return (p[0], p[1], p[2]) + ((0, 0) if p[3] is None else tuple(p[3]))


class PalmCase:
    def __init__(self, name, data, params):
        self.name = name
        self.data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1, 8)
        self.params = _params(params)
        self._expected = None
        assert not R.near_tie(R.palm_trig64(self.data, self.params[0])).any(), name

    @property
    def N(self):
        return self.data.shape[0]

    def expected(self):
        if self._expected is None:
            self._expected = R.palm_decode(self.data, *self.params)
            self._expected.setflags(write=False)
        return self._expected

    def __repr__(self):
        return "PalmCase(%s)" % self.name


class LandmarkCase:
    def __init__(self, name, data, scores, params):
        self.name = name
        self.data = np.ascontiguousarray(data, dtype=np.float32)
        assert self.data.ndim == 2 and self.data.shape[1] % 21 == 0
        self.scores = None if scores is None else np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
        self.params = _params(params)
        self._expected = None
        assert not R.near_tie(R.landmarks_trig64(self.data, self.scores, self.params[0])).any(), name

    @property
    def H(self):
        return self.data.shape[0]

    @property
    def D(self):
        return self.data.shape[1] // 21

    def expected(self):
        if self._expected is None:
            dets, kps = R.landmarks_decode(self.data, self.scores, *self.params)
            dets.setflags(write=False)
            kps.setflags(write=False)
            self._expected = (dets, kps)
        return self._expected

    def __repr__(self):
        return "LandmarkCase(%s)" % self.name


# ---------------------------------------------------------------- palm: synthetic rows

def palm_synth(seed, N):
    """kp0 in U(0.1, 0.9)^2, size in U(0.03, 0.5), kp2 = kp0 + span * (cos a, sin a) with span = size * U(0.1, 1.8), centre in
    U(-0.1, 1.1)^2, uniform scores: about 42 % of such rows pass the validity test."""
    rng = np.random.default_rng(seed)
    kp0 = rng.uniform(0.1, 0.9, (N, 2))
    size = rng.uniform(0.03, 0.5, N)
    a = rng.uniform(0, 2 * np.pi, N)
    span = size * rng.uniform(0.1, 1.8, N)
    kp2 = kp0 + span[:, None] * np.stack([np.cos(a), np.sin(a)], axis=1)
    centre = rng.uniform(-0.1, 1.1, (N, 2))
    score = rng.uniform(0, 1, N)
    return np.concatenate([score[:, None], centre, size[:, None], kp0, kp2], axis=1).astype(np.float32)


def valid_scores(data, frame=None):
    """The scores of the rows that pass every test but the score's, descending."""
    return np.sort(R.palm_candidates(data, -1.0, frame)[1])[::-1]


def threshold_for(data, k):
    """The confidence threshold under which exactly k rows survive the candidate rules (scores are distinct)."""
    s = valid_scores(data)
    assert 0 < k <= len(s) and (k == len(s) or s[k] < s[k - 1])
    return float(s[k - 1])


_PALM_RANDOM = None


def palm_random():
    """N = 0, 1, 63, 64, 65, 255, 256, 257, 2016, 4096 with thresholds that put the survivor count below, on and above a power of two
    and above 64 (more than one selection chunk), over the three frame settings, max_hands 1..8 and several NMS thresholds."""
    global _PALM_RANDOM
    if _PALM_RANDOM is not None:
        return _PALM_RANDOM
    plan = [(0, [None]), (1, [None]), (63, [None]), (64, [None, 16]), (65, [None, 15, 17]), (255, [31, 32, 33, 64]), (256, [63, 65, None]),
            (257, [None, 1]), (2016, [127, 128, 129, 512, None]), (4096, [1023, 1024, 1025, None])]
    cases, k_case = [], 0
    for N, ks in plan:
        data = palm_synth(1000 + N, N)
        if N == 1:
            data[0] = (0.9, 0.5, 0.5, 0.2, 0.5, 0.6, 0.5, 0.5)    # valid: the lone row is a hand
        for k in ks:
            thr = -1.0 if k is None or N == 0 else threshold_for(data, k)
            frame = FRAMES[k_case % 3]
            max_hands = 1 + (k_case * 3) % 8
            iou = (0.08, 0.0, 0.3, 0.6, 1.0)[k_case % 5]
            cases.append(PalmCase("random_N%d_k%s" % (N, k), data, (thr, iou, max_hands, frame)))
            k_case += 1
    # a low NMS threshold over many survivors: the walk goes on through several chunks before max_hands is reached
    data = palm_synth(77, 2016)
    cases.append(PalmCase("random_long_walk", data, (-1.0, 0.0, 8, (640, 360))))
    _PALM_RANDOM = cases
    return cases


# ---------------------------------------------------------------- palm: written-out rows

def palm_row(score, cx, cy, size, kp0=(0.5, 0.5), d=(0.0, -0.5)):
    """kp2 = kp0 + size * d: d = (0, -0.5) is a hand pointing up (rotation 0), span ratio 0.5."""
    return (score, cx, cy, size, kp0[0], kp0[1], kp0[0] + size * d[0], kp0[1] + size * d[1])


def palm_grid(n, score=lambda k: 0.5 + 0.4 * k / 128.0, size=0.03):
    """n valid rows whose boxes (rr = 0.087) sit on a 10 x 10 grid and do not overlap."""
    return np.array([palm_row(score(k), 0.05 + 0.1 * (k % 10), 0.08 + 0.1 * (k // 10), size) for k in range(n)], np.float32)


def palm_written():
    cases = []
    grid = palm_grid(100)
    cases.append(PalmCase("all_dropped", grid, (2.0, 0.3, 8, None)))
    stacked = np.array([palm_row(0.3 + 0.005 * k, 0.5, 0.6, 0.2) for k in range(100)], np.float32)       # one box a hundred times
    for mh in (1, 8):
        cases.append(PalmCase("all_valid_iou1_max%d" % mh, stacked, (0.0, 1.0, mh, (192, 192))))
        cases.append(PalmCase("all_valid_iou_above1_max%d" % mh, stacked, (0.0, 7.5, mh, None)))        # clamped to 1
    cases.append(PalmCase("stacked_iou0", stacked, (0.0, -3.0, 8, None)))                                # clamped to 0: one hand
    equal = palm_grid(70, score=lambda k: 0.75)
    cases.append(PalmCase("equal_scores", equal, (0.5, 0.3, 8, (640, 360))))
    mixed = palm_grid(70, score=lambda k: (0.75, 0.5, 0.75, 0.9)[k % 4])
    cases.append(PalmCase("equal_scores_interleaved", mixed[::-1].copy(), (0.5, 0.3, 8, None)))
    nan = palm_grid(12)
    nan[3, 0], nan[7, 0], nan[9, 0] = bits(QNAN_POS), bits(QNAN_NEG), np.inf
    cases.append(PalmCase("nan_scores", nan, (0.6, 0.3, 8, None)))
    cases.append(PalmCase("nan_threshold", nan, (float("nan"), float("nan"), 8, (192, 192))))
    sizes = palm_grid(8)
    sizes[1, 3], sizes[2, 3], sizes[3, 3], sizes[4, 3], sizes[5, 3] = 0.0, -1.0, np.inf, -0.0, np.nan
    cases.append(PalmCase("bad_sizes", sizes, (0.0, 0.3, 8, None)))
    kps = palm_grid(8)
    kps[1, 4], kps[2, 5], kps[3, 6], kps[4, 7], kps[5, 1], kps[6, 2] = np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan
    cases.append(PalmCase("non_finite_fields", kps, (0.0, 0.3, 8, None)))
    # rotation = FRAC_PI_2 (kp2 right of kp0): sin rounds to 1, so center_x = cx + 0.125 at size 0.25, exactly
    edge = np.array([palm_row(0.9 - 0.01 * k, cx, 0.5, 0.25, d=(0.5, 0.0)) for k, cx in
                     enumerate((-0.125, 0.875, down(-0.125), up(0.875), -0.0625, 0.8125))], np.float32)
    cases.append(PalmCase("centre_on_the_edges", edge, (0.0, 1.0, 8, None)))
    cases.append(PalmCase("centre_on_the_edges_frame", edge, (0.0, 1.0, 8, (640, 360))))
    # rotation 0 (kp2 above kp0): cos rounds to 1, center_y = cy - 0.125 at size 0.25
    edge_y = np.array([palm_row(0.9 - 0.01 * k, 0.5, cy, 0.25) for k, cy in enumerate((0.125, 1.125, down(0.125), up(1.125)))], np.float32)
    cases.append(PalmCase("centre_on_the_edges_y", edge_y, (0.0, 1.0, 8, (192, 192))))
    ranges = np.array([palm_row(0.9, 0.5, 0.5, s) for s in (0.02, 0.0207, 0.4827, 0.483, 0.5)]
                      + [palm_row(0.8, 0.5, 0.5, 0.1, d=(0.0, -r)) for r in (0.1499, 0.15, 0.1501, 1.5999, 1.6, 1.6001, 0.0)], np.float32)
    cases.append(PalmCase("range_ends", ranges, (0.0, 1.0, 8, None)))
    return cases


def palm_iou_pair():
    """Two overlapping hands: the NMS threshold exactly at their IoU keeps both (the test is a strict >), one f32 below drops one."""
    rows = np.array([palm_row(0.9, 0.40, 0.5, 0.1), palm_row(0.8, 0.52, 0.53, 0.12)], np.float32)
    out = []
    for frame in (None, (640, 360)):
        c = R.palm_candidates(rows, 0.0, frame)
        boxes = np.stack(c[3:], axis=1)
        v = R.iou(boxes[0], boxes[1])
        assert len(boxes) == 2 and F32(0.05) < v < F32(0.95)
        out.append((PalmCase("iou_at_threshold_%s" % (frame,), rows, (0.0, float(v), 8, frame)), 2))
        out.append((PalmCase("iou_below_threshold_%s" % (frame,), rows, (0.0, float(down(v)), 8, frame)), 1))
    return out


def centre_edge_facts():
    """(center_x of the six rows of centre_on_the_edges) as the contract computes them."""
    size, rot = F32(0.25), R.FRAC_PI_2 + F32(R.atan2_64(F32(0.0), F32(0.125)))
    t = (F32(0.5) * size) * F32(R.sin_64(rot))
    return [F32(cx) + t for cx in (F32(-0.125), F32(0.875), down(-0.125), up(0.875))]


# ---------------------------------------------------------------- landmarks

def hand_synth(rng, H, D, frame=(640, 360)):
    centre = rng.uniform(0, 1, (H, 1, 2)) * np.array(frame, np.float64)
    scale = rng.uniform(20, 120, (H, 1, 1))
    pts = np.zeros((H, 21, D))
    pts[:, :, :2] = centre + scale * rng.uniform(-0.5, 0.5, (H, 21, 2))
    if D >= 3:
        pts[:, :, 2:] = rng.uniform(0, 1, (H, 21, D - 2))
    return pts.reshape(H, 21 * D).astype(np.float32)


_LM_RANDOM = None


def landmarks_random():
    """H = 0, 1, 2, 11, 65, 1024 with D = 2, 3, 4: scores absent, shorter than H and longer than H (1024: as long)."""
    global _LM_RANDOM
    if _LM_RANDOM is not None:
        return _LM_RANDOM
    cases, k = [], 0
    for H in (0, 1, 2, 11, 65, 1024):
        for D in (2, 3, 4):
            rng = np.random.default_rng(2000 + 10 * H + D)
            data = hand_synth(rng, H, D)
            for kind in ("absent", "short", "full") if H > 1 else ("absent", "full"):
                scores = None if kind == "absent" else rng.uniform(0, 1, H // 2 if kind == "short" else min(H + 3, 1024)).astype(np.float32)
                iou = (0.2, 0.0, 0.5, 1.5, -1.0)[k % 5]
                cases.append(LandmarkCase("random_H%d_D%d_%s" % (H, D, kind), data, scores, (0.5, iou, 1 + (k * 3) % 10, FRAMES[1 + k % 2])))
                k += 1
    _LM_RANDOM = cases
    return cases


def hand_box(x0, y0, x1, y1, D=3, conf=0.9):
    """A hand whose 21 points span exactly (x0, y0)-(x1, y1): wrist bottom centre, middle-finger base above it."""
    p = np.zeros((21, D), np.float32)
    t = np.linspace(0.0, 1.0, 21)
    p[:, 0] = x0 + (x1 - x0) * t
    p[:, 1] = y0 + (y1 - y0) * ((np.arange(21) * 7) % 21) / 20.0
    p[0, :2] = ((x0 + x1) / 2, y1)
    p[9, :2] = ((x0 + x1) / 2 + 1.0, (y0 + y1) / 2)
    p[1, :2], p[2, :2] = (x0, y0), (x1, y1)
    if D >= 3:
        p[:, 2:] = conf
    return p.reshape(-1)


def landmarks_written():
    nan, inf = np.nan, np.inf
    cases = []
    for D in (2, 3, 4):
        hands = np.stack([hand_box(40 + 150 * k, 30, 140 + 150 * k, 200, D) for k in range(6)])
        h = hands.reshape(6, 21, D)
        h[0, :, :2] = nan                                   # no finite point: dropped
        h[1, 1:, 0] = inf                                   # one finite point: a degenerate box, dropped
        h[2, 0, 0] = nan                                    # wrist not finite: the rotation is NaN and passes through
        h[3, 0, 1] = inf                                    # atan2(-inf, 1)
        h[4, 5, 1], h[4, 7, 0], h[4, 20, 0] = nan, -inf, nan  # three points skipped: the keypoint record is compacted
        if D >= 3:
            h[5, :6, 2] = (0.5, up(0.5), down(0.5), nan, inf, -1.0)
        for scores in (None, [0.6, 0.7, 0.8]):
            cases.append(LandmarkCase("special_D%d_%s" % (D, "absent" if scores is None else "short"), hands, scores, (0.5, 0.2, 10, (1000, 360))))
    # A lies wholly right of the 640 x 360 frame: no oriented box, but it suppresses B and counts toward max_hands = 2
    out = np.stack([hand_box(700, 50, 800, 150), hand_box(690, 60, 790, 160), hand_box(100, 50, 200, 150), hand_box(300, 50, 400, 150)])
    for mh, iou in ((2, 0.2), (4, 0.2), (4, 0.9)):
        cases.append(LandmarkCase("outside_frame_max%d_iou%s" % (mh, iou), out, [0.9, 0.8, 0.7, 0.6], (0.5, iou, mh, (640, 360))))
    cases.append(LandmarkCase("no_frame", out, [0.9, 0.8, 0.7, 0.6], (0.5, 0.2, 4, None)))
    cases.append(LandmarkCase("nan_settings", out, [0.9, nan, bits(QNAN_NEG), 0.6], (nan, nan, 10, (640, 360))))
    big = np.stack([hand_box(-3e38, -3e38, 3e38, 3e38), hand_box(-3e9, 5, 3e9, 50), hand_box(10.5, 20.5, 10.75, 20.75), hand_box(-0.0, -0.0, 0.5, 0.25)])
    cases.append(LandmarkCase("huge_and_tiny", big, None, (0.5, 0.2, 10, (640, 360))))
    return cases


def landmarks_iou_pair():
    hands = np.stack([hand_box(100, 100, 200, 200), hand_box(150, 120, 260, 230)])
    dets, _ = R.landmarks_decode(hands, [0.9, 0.8], 0.5, 2.0, 10, (640, 360))
    box = lambda d: (d["xmin"], d["ymin"], d["xmax"], d["ymax"])
    v = R.iou(box(dets[0]), box(dets[1]))
    assert len(dets) == 2 and F32(0.05) < v < F32(0.95)
    return [(LandmarkCase("iou_at_threshold", hands, [0.9, 0.8], (0.5, float(v), 10, (640, 360))), 2),
            (LandmarkCase("iou_below_threshold", hands, [0.9, 0.8], (0.5, float(down(v)), 10, (640, 360))), 1)]


def palm_all():
    return palm_random() + palm_written() + [c for c, _ in palm_iou_pair()]


def landmarks_all():
    return landmarks_random() + landmarks_written() + [c for c, _ in landmarks_iou_pair()]
