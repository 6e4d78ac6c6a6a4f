"""Helpers for the BF16 precision of yoloxinference's network (mi355_yolox_net_set_precision) - no tests here.

bf16_round            round to nearest, ties to even, on the f32 bit pattern, in numpy integers.
bf16_operands(dtype)  a context manager under which yolox_net_restate.conv2d rounds x and w of every DENSE convolution (groups == 1)
                      to bf16 and sums in `dtype`; depthwise convolutions pass through. Under it Yolox.forward is the bf16-operand
                      restatement: what a BF16 net computes, up to the order of its sums.
references(case)      per case of yolox_net_cases.all_cases(): ref64 (the existing f64 maps), emu64 (bf16 operands, everything else f64)
                      and emu32 (bf16 operands, everything else f32), each computed once for a (config, classes, shape) and shared.
pooled_rms            the statistic: the RMS error against ref64 pooled over the three levels, all maps and the case's frames.
bf16_cases()          the cases whose two emulations agree: rms(emu32 - ref64) / rms(emu64 - ref64) in [0.6, 1.5] - where f32
                      accumulation noise, not the operand rounding, decides the error, the f64 emulation is no yardstick for a device
                      that sums in f32. At most 4 of the 40 cases may go; the helper asserts it, so the guard cannot empty the test."""
import contextlib
import functools

import numpy as np

import yolox_net_cases as K
import yolox_net_restate as R

GUARD = (0.6, 1.5)
MAX_DROPPED = 4


def bf16_round(a):
    """f32 array -> the f32 array of its values rounded to bf16 (nearest, ties to even): finite values below 2^127."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (bits + np.uint64(0x7FFF) + ((bits >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return (r << np.uint64(16)).astype(np.uint32).view(np.float32).reshape(np.shape(a))


def bf16_bits(a):
    """the 16-bit patterns of bf16_round(a)"""
    return (bf16_round(a).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


@contextlib.contextmanager
def bf16_operands(dtype):
    original = R.conv2d

    def conv2d(x, w, stride=1, pad=0, groups=1, bias=None):
        if groups != 1:
            return original(x, w, stride, pad, groups, bias)
        out = original(bf16_round(x.astype(np.float32)).astype(dtype), bf16_round(w.astype(np.float32)).astype(dtype), stride, pad, groups, bias)
        return out.astype(x.dtype)

    R.conv2d = conv2d
    try:
        yield
    finally:
        R.conv2d = original


@functools.lru_cache(maxsize=None)
def _emulations(config, num_classes, H, W):
    """{dtype name: maps of the three frames} under bf16 operands"""
    case = K.Case(config, num_classes, H, W, 3)
    x = R.input_tensor(case.frames)
    P = case.P                  # the seeded set and its references are built lazily: never under the patch
    case.ref(np.float64)
    out = {}
    for dt in (np.float64, np.float32):
        with bf16_operands(dt):
            maps = case.net.forward(P, x, dt)
        for m in maps:
            m.setflags(write=False)
        out[np.dtype(dt).name] = maps
    return out


def references(case):
    """(ref64, emu64, emu32): per level [n, 5 + C, h, w]; a batch of one is the first frame of the batch of three"""
    emu = _emulations(case.config, case.C, case.H, case.W)
    return case.ref(np.float64), [m[:case.n] for m in emu["float64"]], [m[:case.n] for m in emu["float32"]]


def pooled_rms(maps, ref64):
    sq = sum(float(((np.asarray(m, np.float64) - r) ** 2).sum()) for m, r in zip(maps, ref64))
    return float(np.sqrt(sq / sum(r.size for r in ref64)))


def guard_ratio(case):
    ref64, emu64, emu32 = references(case)
    return pooled_rms(emu32, ref64) / pooled_rms(emu64, ref64)


@functools.lru_cache(maxsize=None)
def _guarded():
    cases = K.all_cases()
    kept, dropped = [], []
    for c in cases:
        ratio = guard_ratio(c)
        (kept if GUARD[0] <= ratio <= GUARD[1] else dropped).append((c, ratio))
    assert len(dropped) <= MAX_DROPPED, [(c.name, r) for c, r in dropped]
    return tuple(kept), tuple(dropped)


def bf16_cases():
    return [c for c, _ in _guarded()[0]]
