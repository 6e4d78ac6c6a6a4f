"""numpy restatement of the yolov8tensordec2 / yoloxtensordec decode contract (the reference loop is
analytics/analytics/src/yolotensordec/imp.rs:234-422 with iou at :480-489). f32 throughout, one function per rule, written from
the contract and not from the kernels. The checker of tests/test_yolodec_cpu.py and tests/test_gpu_yolodec.py.

    decode(data, layout, box_thr, class_thr, iou_thr) -> DET record array in output order

data: float32, shape (F, N) for layout "V8" (field f of candidate c is data[f, c]) and (N, F) for "X" (candidate c is data[c])."""
import numpy as np

DET = np.dtype([("xmin", "<f4"), ("ymin", "<f4"), ("xmax", "<f4"), ("ymax", "<f4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"),
                ("height", "<i4"), ("class_id", "<u4"), ("confidence", "<f4"), ("candidate", "<u4"), ("reserved", "<u4")])

F32 = np.float32
ONE, TWO, ZERO = F32(1.0), F32(2.0), F32(0.0)


def total_key(x):
    """f32::total_cmp as an integer order: bits ^ ((bits >>arith 31) >>logical 1), compared as i32."""
    s = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return s ^ ((s >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)


def argmax_last(scores):
    """Rule 1/2: per column of scores (classes, n) the maximum under total_cmp, the LAST of equal maxima (Iterator::max_by)."""
    k = total_key(scores)
    n_classes = k.shape[0]
    return (n_classes - 1 - np.argmax(k[::-1], axis=0)).astype(np.uint32)


def candidates(data, layout, box_thr, class_thr):
    """Rules 1-3 -> (candidate index, class, confidence, xmin, ymin, xmax, ymax) of the candidates that stay, in tensor order."""
    data = np.ascontiguousarray(data, dtype=np.float32)
    box_thr, class_thr = F32(box_thr), F32(class_thr)
    with np.errstate(all="ignore"):
        if layout == "V8":
            x, y, w, h = data[0], data[1], data[2], data[3]
            scores = data[4:]
            n = data.shape[1]
            cls = argmax_last(scores) if n else np.zeros(0, np.uint32)
            conf = scores[cls, np.arange(n)]
            keep = ~(conf < class_thr)
            confidence = conf
        elif layout == "X":
            x, y, w, h, obj = data[:, 0], data[:, 1], data[:, 2], data[:, 3], data[:, 4]
            scores = data[:, 5:].T
            n = data.shape[0]
            cls = argmax_last(scores) if n else np.zeros(0, np.uint32)
            conf = scores[cls, np.arange(n)]
            keep = ~(obj < box_thr) & ~(conf < class_thr)
            confidence = (obj * conf).astype(np.float32)
        else:
            raise ValueError(layout)
        xmin, ymin = x - w / TWO, y - h / TWO
        xmax, ymax = x + w / TWO, y + h / TWO
    idx = np.nonzero(keep)[0].astype(np.uint32)
    return idx, cls[idx], confidence[idx], xmin[idx], ymin[idx], xmax[idx], ymax[idx]


def order(idx, cls, confidence):
    """Rule 4: class ascending, confidence descending under total_cmp, candidate index ascending (the defined tie order)."""
    return np.lexsort((idx, ~total_key(confidence), cls))


def iou_kept(kx0, ky0, kx1, ky1, x0, y0, x1, y1):
    """Rule 5's iou with the kept boxes (arrays) as the first operand and the tested box (scalars) as the second."""
    with np.errstate(all="ignore"):
        a1 = (kx1 - kx0 + ONE) * (ky1 - ky0 + ONE)
        a2 = (x1 - x0 + ONE) * (y1 - y0 + ONE)
        ix0, ix1 = np.fmax(kx0, x0), np.fmin(kx1, x1)
        iy0, iy1 = np.fmax(ky0, y0), np.fmin(ky1, y1)
        ia = np.fmax(ix1 - ix0 + ONE, ZERO) * np.fmax(iy1 - iy0 + ONE, ZERO)
        return ia / (a1 + a2 - ia)


def nms_run(xmin, ymin, xmax, ymax, iou_thr):
    """Rule 5 over one class run in sorted order -> positions kept."""
    n = len(xmin)
    kept = np.zeros(n, np.int64)
    kb = np.zeros((4, n), np.float32)
    m = 0
    for i in range(n):
        if m and (iou_kept(kb[0, :m], kb[1, :m], kb[2, :m], kb[3, :m], xmin[i], ymin[i], xmax[i], ymax[i]) > iou_thr).any():
            continue
        kb[:, m] = (xmin[i], ymin[i], xmax[i], ymax[i])
        kept[m] = i
        m += 1
    return kept[:m]


def cast_i32(v):
    """Rust's `as i32`: toward zero, saturating, NaN -> 0."""
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.int32)
    nan = np.isnan(v)
    hi = ~nan & (v >= F32(2147483648.0))
    lo = ~nan & (v <= F32(-2147483648.0))
    mid = ~(nan | hi | lo)
    out[hi] = np.iinfo(np.int32).max
    out[lo] = np.iinfo(np.int32).min
    out[mid] = np.trunc(v[mid]).astype(np.int64).astype(np.int32)
    return out


def decode(data, layout, box_thr, class_thr, iou_thr):
    idx, cls, conf, xmin, ymin, xmax, ymax = candidates(data, layout, box_thr, class_thr)
    o = order(idx, cls, conf)
    idx, cls, conf, xmin, ymin, xmax, ymax = (a[o] for a in (idx, cls, conf, xmin, ymin, xmax, ymax))
    iou_thr = F32(iou_thr)
    keep = []
    start = 0
    n = len(idx)
    while start < n:
        end = start
        while end < n and cls[end] == cls[start]:
            end += 1
        keep.append(start + nms_run(xmin[start:end], ymin[start:end], xmax[start:end], ymax[start:end], iou_thr))
        start = end
    k = np.concatenate(keep) if keep else np.zeros(0, np.int64)
    out = np.zeros(len(k), DET)
    out["xmin"], out["ymin"], out["xmax"], out["ymax"] = xmin[k], ymin[k], xmax[k], ymax[k]
    with np.errstate(all="ignore"):
        out["x"], out["y"] = cast_i32(xmin[k]), cast_i32(ymin[k])
        out["width"], out["height"] = cast_i32(xmax[k] - xmin[k]), cast_i32(ymax[k] - ymin[k])
    out["class_id"], out["confidence"], out["candidate"] = cls[k], conf[k], idx[k]
    return out


def same_records(a, b, float_boxes_nan_equal=True):
    """Every field bit-equal; the four f32 box fields compare NaN == NaN (rule 8: a produced NaN's payload is the hardware's)."""
    if a.shape != b.shape:
        return False
    for name in DET.names:
        x, y = a[name], b[name]
        if name in ("xmin", "ymin", "xmax", "ymax") and float_boxes_nan_equal:
            same = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        else:
            same = x.view(np.uint32) == y.view(np.uint32)
        if not same.all():
            return False
    return True
