"""numpy restatement of the yoloxinference head decode and input conversion (the reference is Head::forward /
Head::decode, analytics/burn/src/yoloxinference/yolox_burn/model/head.rs:23-34, :74-85, :89-122, and yoloxinference/imp.rs:439-447,
:533-539). Written from the contract and not from the kernels. The checker of tests/test_yolox_head_cpu.py and
tests/test_gpu_yolox_head.py.

    tensor(levels)                                  -> the decoded [A, 5 + C] float32 tensor
    dets(levels, box_thr, class_thr, iou_thr)       -> DET records: yolodec_restate.decode of that tensor, layout "X" (by composition)
    input_tensor(frame, stride, width, height)      -> [3, H, W] float32
    deviation64(levels)                             -> every f64 value behind the stated deviation (for handdec_restate.near_tie)
    fused_xy(levels)                                -> fields 0 and 1 as ONE rounding of (reg + g) * s would give them

levels: a sequence of (reg, obj, cls, stride) with float32 arrays of shape (4, h, w), (1, h, w), (C, h, w) and an integer stride.
Stated deviation: exp and sigmoid are numpy's float64 functions of the f32 argument, rounded once to f32 (RESTATED WITHOUT SOURCE,
PARITY UNPINNED); sign and payload of a NaN are outside the contract (same_tensor, yolodec_restate.same_records)."""
import numpy as np

import yolodec_restate as Y

F32 = np.float32
DET = Y.DET


def exp64(x):
    """The f64 exponential of f32 arguments."""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, np.float32).astype(np.float64))


def sigmoid64(x):
    """1 / (1 + exp(-x)) in f64 from f32 arguments."""
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float32).astype(np.float64)))


def exp32(x):
    with np.errstate(all="ignore"):
        return exp64(x).astype(np.float32)


def sigmoid32(x):
    with np.errstate(all="ignore"):
        return sigmoid64(x).astype(np.float32)


def grid(h, w):
    """(gx, gy) per element i = y * w + x: x is the fast index."""
    i = np.arange(h * w)
    return (i % w).astype(np.float32), (i // w).astype(np.float32)


def level_rows(reg, obj, cls, stride):
    """The rows of one level, [h * w, 5 + C]."""
    reg, obj, cls = (np.asarray(a, np.float32) for a in (reg, obj, cls))
    _, h, w = reg.shape
    n_classes = cls.shape[0]
    r, o, c = reg.reshape(4, h * w), obj.reshape(h * w), cls.reshape(n_classes, h * w)
    gx, gy = grid(h, w)
    s = F32(stride)
    out = np.empty((h * w, 5 + n_classes), np.float32)
    with np.errstate(all="ignore"):
        out[:, 0] = (r[0] + gx).astype(np.float32) * s        # the add is rounded to f32 before the multiply
        out[:, 1] = (r[1] + gy).astype(np.float32) * s
        out[:, 2] = exp32(r[2]) * s
        out[:, 3] = exp32(r[3]) * s
        out[:, 4] = sigmoid32(o)
        out[:, 5:] = sigmoid32(c).T
    return out


def tensor(levels):
    return np.concatenate([level_rows(*lv) for lv in levels], axis=0)


def dets(levels, box_thr, class_thr, iou_thr, decoded=None):
    return Y.decode(tensor(levels) if decoded is None else decoded, "X", box_thr, class_thr, iou_thr)


def deviation64(levels):
    vals = []
    for reg, obj, cls, _ in levels:
        reg = np.asarray(reg, np.float32)
        vals += [exp64(reg[2:4]).reshape(-1), sigmoid64(obj).reshape(-1), sigmoid64(cls).reshape(-1)]
    return np.concatenate(vals)


def fused_xy(levels):
    """Fields 0 and 1 with the add and the multiply rounded ONCE (exact in f64 for these magnitudes, then one conversion)."""
    out = []
    for reg, _, _, stride in levels:
        reg = np.asarray(reg, np.float32)
        _, h, w = reg.shape
        gx, gy = grid(h, w)
        r = reg.reshape(4, h * w).astype(np.float64)
        out.append(np.stack([((r[0] + gx) * float(stride)).astype(np.float32), ((r[1] + gy) * float(stride)).astype(np.float32)], axis=1))
    return np.concatenate(out, axis=0)


def input_tensor(frame, stride, width, height):
    """frame: uint8 bytes of one frame; out[c][y][x] = (f32) frame[y * stride + 3 x + c]."""
    frame = np.asarray(frame, np.uint8).reshape(-1)
    out = np.empty((3, height, width), np.float32)
    for y in range(height):
        row = frame[y * stride: y * stride + 3 * width].reshape(width, 3)
        out[:, y, :] = row.T
    return out


def same_tensor(a, b):
    """Bit-equal, NaN == NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


same_records = Y.same_records
