"""numpy restatement of the handdetectiontensordec / handlandmarktensordec decode contract (the reference loops are
analytics/analytics/src/hand/handdetectiontensordec/imp.rs:89-335, hand/handlandmarktensordec/imp.rs:101-391 and
hand/helper.rs:69-114). f32 throughout and unfused, one function per rule, written from the contract and not from the kernels.
The checker of tests/test_handdec_cpu.py and tests/test_gpu_handdec.py.

    palm_decode(data, conf_thr, iou_thr, max_hands, frame=None)                      -> DET records in output order
    landmarks_decode(data, scores, conf_thr, iou_thr, max_hands, frame=None)         -> (DET records, KP records)
    palm_trig64(data, conf_thr) / landmarks_trig64(data, scores, conf_thr)           -> the f64 values behind deviation a
    near_tie(v64, ulps=16)                                                           -> which of them lie at an f32 rounding midpoint

data: float32, (N, 8) palm rows score, cx, cy, size, kp0x, kp0y, kp2x, kp2y; (H, 21 * D) landmarks. frame: (width, height) or None.
Deviation a: atan2 / sin / cos are numpy's float64 functions of the f32 arguments, rounded once to f32. Deviation b: iou is restated
without source, parity unpinned. Deviation c: sign and payload of a produced NaN are outside the contract (same_records)."""
import numpy as np

DET = np.dtype([("xmin", "<f4"), ("ymin", "<f4"), ("xmax", "<f4"), ("ymax", "<f4"), ("rotation", "<f4"), ("rotation_od", "<f4"),
                ("confidence", "<f4"), ("index", "<u4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("has_od", "<u4"),
                ("reserved", "<u4", (3,))])
KP = np.dtype([("count", "<u4"), ("positions", "<i4", (42,)), ("confidences", "<f4", (21,)), ("visibilities", "u1", (21,)), ("reserved", "u1", (11,))])
KP_UNKNOWN, KP_VISIBLE, KP_OCCLUDED = 0, 1, 2

F32 = np.float32
ZERO, ONE, TWO, HALF = F32(0.0), F32(1.0), F32(2.0), F32(0.5)
FRAC_PI_2 = F32(np.pi / 2)
PALM_MIN_RR, PALM_MAX_RR = F32(0.06), F32(1.40)
PALM_MIN_SPAN, PALM_MAX_SPAN = F32(0.15), F32(1.60)
PALM_MIN_VISIBLE = F32(0.5)
RR_SCALE = F32(2.9)
HAND_PAD = F32(0.15)


def total_key(x):
    """f32::total_cmp as an integer order: bits ^ ((bits >>arith 31) >>logical 1), compared as i32."""
    s = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return s ^ ((s >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)


def near_tie(v64, ulps=16):
    """Deviation a's guard: True where the f64 value lies within `ulps` f64 ULP of the midpoint of two neighbouring f32 values -
    where two f64 libms whose error is below that may round to different f32 values. Non-finite values are never flagged."""
    v = np.atleast_1d(np.asarray(v64, np.float64))
    out = np.zeros(v.shape, bool)
    ok = np.isfinite(v)
    with np.errstate(all="ignore"):
        r = v[ok].astype(np.float32)
        up = np.nextafter(r, F32(np.inf)).astype(np.float64)
        dn = np.nextafter(r, F32(-np.inf)).astype(np.float64)
        r64 = r.astype(np.float64)
        d = np.minimum(np.abs(v[ok] - (r64 + up) / 2), np.abs(v[ok] - (r64 + dn) / 2))
        out[ok] = d <= ulps * np.spacing(np.abs(v[ok]))
    return out


def atan2_64(y, x):
    return np.arctan2(np.asarray(y, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64))


def sin_64(v):
    return np.sin(np.asarray(v, np.float32).astype(np.float64))


def cos_64(v):
    return np.cos(np.asarray(v, np.float32).astype(np.float64))


def cast_i32(f):
    """Rust's `as i32` of one f32: toward zero, saturating, NaN -> 0."""
    f = F32(f)
    if np.isnan(f):
        return 0
    if f >= F32(2147483648.0):
        return 2147483647
    if f <= F32(-2147483648.0):
        return -2147483648
    return int(np.trunc(f))


def iou(a, b):
    """Deviation b. a, b: (xmin, ymin, xmax, ymax) of f32 scalars."""
    with np.errstate(all="ignore"):
        aw, ah, bw, bh = a[2] - a[0], a[3] - a[1], b[2] - b[0], b[3] - b[1]
        iw = np.fmax(ZERO, np.fmin(a[0] + aw, b[0] + bw) - np.fmax(a[0], b[0]))
        ih = np.fmax(ZERO, np.fmin(a[1] + ah, b[1] + bh) - np.fmax(a[1], b[1]))
        inter = F32(iw * ih)
        union = F32(F32(F32(aw * ah) + F32(bw * bh)) - inter)
        return F32(inter / union) if union > ZERO else ZERO


def oriented_od(box, rotation, frame):
    """helper.rs:69-114 -> (x, y, width, height, rotation_od) or None."""
    x0, y0, x1, y1 = (F32(v) for v in box)
    if not all(np.isfinite(v) for v in (x0, y0, x1, y1)):
        return None
    x0, y0, x1, y1 = np.floor(x0), np.floor(y0), np.ceil(x1), np.ceil(y1)
    if x1 <= x0 or y1 <= y0:
        return None
    if frame is not None and frame[0] > 0 and frame[1] > 0:
        fw, fh = F32(frame[0]), F32(frame[1])
        if x1 <= ZERO or y1 <= ZERO or x0 >= fw or y0 >= fh:
            return None
    with np.errstate(all="ignore"):
        x, y, w, h = cast_i32(x0), cast_i32(y0), cast_i32(F32(x1 - x0)), cast_i32(F32(y1 - y0))
        if w <= 0 or h <= 0:
            return None
        return x, y, w, h, F32(F32(rotation) + (-FRAC_PI_2))


def _palm_pass(data, conf_thr):
    """Rule 1: rows that stay after the score and the size test."""
    with np.errstate(all="ignore"):
        return np.nonzero(~(data[:, 0] < F32(conf_thr)) & ~(data[:, 3] <= ZERO))[0]


def palm_trig64(data, conf_thr):
    """The f64 atan2, sin and cos values of the rows that passed rule 1, concatenated."""
    data = np.ascontiguousarray(data, np.float32).reshape(-1, 8)
    r = data[_palm_pass(data, conf_thr)]
    with np.errstate(all="ignore"):
        a = atan2_64(r[:, 7] - r[:, 5], r[:, 6] - r[:, 4])
        rot = FRAC_PI_2 + a.astype(np.float32)
        return np.concatenate([a, sin_64(rot), cos_64(rot)])


def palm_candidates(data, conf_thr, frame):
    """Rules 1-6 -> (row index, score, rotation, xmin, ymin, xmax, ymax) of the rows that stay, in tensor order."""
    data = np.ascontiguousarray(data, np.float32).reshape(-1, 8)
    idx = _palm_pass(data, conf_thr)
    r = data[idx]
    score, cx, cy, size, k0x, k0y, k2x, k2y = (r[:, k] for k in range(8))
    with np.errstate(all="ignore"):
        dx, dy = k2x - k0x, k2y - k0y
        rot = FRAC_PI_2 + atan2_64(dy, dx).astype(np.float32)
        rr = RR_SCALE * size
        ctx = cx + (HALF * size) * sin_64(rot).astype(np.float32)
        cty = cy - (HALF * size) * cos_64(rot).astype(np.float32)
        ok = np.isfinite(ctx) & np.isfinite(cty) & np.isfinite(rr) & np.isfinite(size) & np.isfinite(k0x) & np.isfinite(k0y) & np.isfinite(k2x) & np.isfinite(k2y)
        ok &= (PALM_MIN_RR <= rr) & (rr <= PALM_MAX_RR)
        ok &= (ZERO <= ctx) & (ctx <= ONE) & (ZERO <= cty) & (cty <= ONE)
        ratio = np.sqrt(dx * dx + dy * dy) / size
        ok &= (PALM_MIN_SPAN <= ratio) & (ratio <= PALM_MAX_SPAN)
        hs = rr * HALF
        x0, y0, x1, y1 = ctx - hs, cty - hs, ctx + hs, cty + hs
        area = np.fmax(x1 - x0, ZERO) * np.fmax(y1 - y0, ZERO)
        ok &= ~(area <= ZERO)
        inter = np.fmax(np.fmin(x1, ONE) - np.fmax(x0, ZERO), ZERO) * np.fmax(np.fmin(y1, ONE) - np.fmax(y0, ZERO), ZERO)
        ok &= (inter / area) >= PALM_MIN_VISIBLE
        if frame is not None:
            w, h = F32(frame[0]), F32(frame[1])
            ctx, cty, rr = ctx * w, cty * h, rr * np.fmax(w, h)
        half = rr / TWO
        cols = (idx.astype(np.uint32), score, rot, ctx - half, cty - half, ctx + half, cty + half)
    assert all(c.dtype in (np.float32, np.uint32) for c in cols)
    return tuple(c[ok] for c in cols)


def order(idx, score):
    """Rule 7: score descending under total_cmp, index ascending among equal keys (a stable sort)."""
    return np.lexsort((idx, ~total_key(score)))


def select(boxes, thr, max_hands):
    """Rule 8 over the sorted boxes (n, 4) -> positions kept."""
    kept = []
    for i in range(len(boxes)):
        if any(iou(boxes[i], boxes[j]) > thr for j in kept):
            continue
        kept.append(i)
        if len(kept) >= max_hands:
            break
    return kept


def _records(idx, conf, rot, boxes, kept, frame):
    out = np.zeros(len(kept), DET)
    for o, k in enumerate(kept):
        d = out[o]
        d["xmin"], d["ymin"], d["xmax"], d["ymax"] = boxes[k]
        d["rotation"], d["confidence"], d["index"] = rot[k], conf[k], idx[k]
        od = oriented_od(boxes[k], rot[k], frame)
        if od is not None:
            d["x"], d["y"], d["width"], d["height"], d["rotation_od"] = od
            d["has_od"] = 1
    return out


def clamp01(t):
    """f32::clamp(0, 1): a NaN stays."""
    t = F32(t)
    return ZERO if t < ZERO else ONE if t > ONE else t


def palm_decode(data, conf_thr, iou_thr, max_hands, frame=None):
    idx, score, rot, x0, y0, x1, y1 = palm_candidates(data, conf_thr, frame)
    o = order(idx, score)
    idx, score, rot = idx[o], score[o], rot[o]
    boxes = np.stack([x0[o], y0[o], x1[o], y1[o]], axis=1) if len(o) else np.zeros((0, 4), np.float32)
    kept = select(boxes, clamp01(iou_thr), max_hands)
    return _records(idx, score, rot, boxes, kept, frame)


def _hand_conf(H, scores):
    conf = np.ones(H, np.float32)
    if scores is not None:
        s = np.ascontiguousarray(scores, np.float32).reshape(-1)
        n = min(H, len(s))
        conf[:n] = s[:n]
    return conf


def landmarks_trig64(data, scores, conf_thr):
    """The f64 atan2 values of the hands that passed the confidence test."""
    data = np.ascontiguousarray(data, np.float32)
    H, D = data.shape[0], data.shape[1] // 21
    conf = _hand_conf(H, scores)
    with np.errstate(all="ignore"):
        p = data.reshape(H, 21, D)[~(conf < F32(conf_thr))]
        return atan2_64(p[:, 9, 1] - p[:, 0, 1], p[:, 9, 0] - p[:, 0, 0])


def landmarks_decode(data, scores, conf_thr, iou_thr, max_hands, frame=None):
    data = np.ascontiguousarray(data, np.float32)
    H = data.shape[0]
    assert data.ndim == 2 and data.shape[1] % 21 == 0 and data.shape[1] // 21 >= 2
    D = data.shape[1] // 21
    pts = data.reshape(H, 21, D)
    conf = _hand_conf(H, scores)
    idx, cf, rot, boxes = [], [], [], []
    with np.errstate(all="ignore"):
        for h in range(H):
            if conf[h] < F32(conf_thr):
                continue
            x, y = pts[h, :, 0], pts[h, :, 1]
            fin = np.isfinite(x) & np.isfinite(y)
            if not fin.any():
                continue
            mnx, mxx, mny, mxy = x[fin].min(), x[fin].max(), y[fin].min(), y[fin].max()
            width, height = F32(mxx - mnx), F32(mxy - mny)
            if width <= ZERO or height <= ZERO:
                continue
            boxes.append((mnx - width * HAND_PAD, mny - height * HAND_PAD, mxx + width * HAND_PAD, mxy + height * HAND_PAD))
            rot.append(FRAC_PI_2 + F32(atan2_64(pts[h, 9, 1] - pts[h, 0, 1], pts[h, 9, 0] - pts[h, 0, 0])))
            idx.append(h)
            cf.append(conf[h])
    idx, cf, rot = np.array(idx, np.uint32), np.array(cf, np.float32), np.array(rot, np.float32)
    boxes = np.array(boxes, np.float32).reshape(-1, 4)
    o = order(idx, cf)
    idx, cf, rot, boxes = idx[o], cf[o], rot[o], boxes[o]
    kept = select(boxes, F32(iou_thr), max_hands)
    dets = _records(idx, cf, rot, boxes, kept, frame)
    kps = np.zeros(len(kept), KP)
    for o_, k in enumerate(kept):
        h, n = int(idx[k]), 0
        for j in range(21):
            x, y = pts[h, j, 0], pts[h, j, 1]
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            kps[o_]["positions"][2 * n], kps[o_]["positions"][2 * n + 1] = cast_i32(x), cast_i32(y)
            if D >= 3:
                c = pts[h, j, 2]
                kps[o_]["confidences"][n] = c
                kps[o_]["visibilities"][n] = KP_VISIBLE if c > HALF else KP_OCCLUDED
            else:
                kps[o_]["confidences"][n] = cf[k]
                kps[o_]["visibilities"][n] = KP_UNKNOWN
            n += 1
        kps[o_]["count"] = n
    return dets, kps


FLOAT_FIELDS = {"xmin", "ymin", "xmax", "ymax", "rotation", "rotation_od", "confidence", "confidences"}


def same_records(a, b):
    """Every field bit-equal; f32 fields compare NaN == NaN (deviation c)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    for name in a.dtype.names:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if name in FLOAT_FIELDS:
            same = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        else:
            same = x == y
        if not np.all(same):
            return False
    return True
