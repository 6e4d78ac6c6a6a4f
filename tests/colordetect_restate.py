"""Independent restatement of colordetect's palette (color-thief 0.2.2 MMCQ, as DESIGN §4.8 states it: parity unpinned) and of
color-name 1.2.0's `css::Color::similar`. Plain Python + numpy, integer arithmetic only: the device must agree bit for bit.
Used by tests/test_colordetect_cpu.py, tests/test_gpu_colordetect.py and, with the branch trace (LABELS), by the directed cases of
tests/colordetect_cases.py; not part of the product."""
import json
import os

import numpy as np

# byte offsets (r, g, b, a) inside one pixel; a = None: opaque (255)
LAYOUT = {"RGB": (3, 0, 1, 2, None), "RGBA": (4, 0, 1, 2, 3), "ARGB": (4, 1, 2, 3, 0), "BGR": (3, 2, 1, 0, None), "BGRA": (4, 2, 1, 0, 3)}
MAX_ITERATIONS = 1000

# One label per decision of _iter and _cut, recorded in the optional `trace` of palette_from_histogram (None: nothing is recorded and
# nothing else changes). "A." / "B." is the phase; besides these there is one "cut.axis.<axis>/<widest axes>" label per cut, e.g.
# "cut.axis.r/rg": r cut, r and g the widest (tests/colordetect_cases.py derives which of them exist).
_PHASE_LABELS = {
    "target_met_on_entry": "size >= target before the first round",
    "target_met_after_cut": "size >= target after a cut",
    "sorted_already": "a pop finds the queue in ascending key order",
    "sorted_again": "a pop finds the queue out of order",
    "equal_keys_on_top": "the two largest keys are equal: the stable order decides which box is popped",
    "count1_top_nothing_cuttable": "a box of count 1 is popped and no other box has count >= 2",
    "count1_top_cuttable_below": "a box of count 1 is popped while a box of count >= 2 stands below it: the phase stalls",
    "count0_top": "a box of count 0 is popped (the round counts twice)",
    "iteration_cap": "the 1000 rounds are spent",
}
LABELS = {"%s.%s" % (ph, k): "phase %s: %s" % (ph, v) for ph in "AB" for k, v in _PHASE_LABELS.items()}
LABELS.update({
    "cut.median.exact_half": "a slice before i has 2 * partial == total exactly (> decides, not >=)",
    "cut.median.left_le_right": "left <= right: d = min(hi - 1, i + right // 2)",
    "cut.median.min_clipped": "... and hi - 1 is the smaller",
    "cut.median.min_unclipped": "... and i + right // 2 is taken",
    "cut.median.left_gt_right": "left > right: d = max(lo, i - 1 - (left + 1) // 2)",
    "cut.median.max_clipped": "... and lo is the larger",
    "cut.median.max_unclipped": "... and i - 1 - (left + 1) // 2 is taken",
    "cut.advance.none": "d stays: d >= lo and partial[d] != 0",
    "cut.advance.d_below_lo": "d rises because d < lo",
    "cut.advance.empty_prefix": "d rises because partial[d] == 0",
    "cut.retreat.not_entered": "the second box is not empty at the first d",
    "cut.retreat.stepped": "d falls one slice and the second box is still empty",
    "cut.retreat.stepped_to_nonempty": "d falls one slice and the second box has samples now",
    "cut.retreat.stopped_at_lo": "the second box stays empty: d is at lo",
    "cut.retreat.stopped_by_empty_prefix": "the second box stays empty: partial[d - 1] == 0",
    "cut.second.nonempty": "second box with samples",
    "cut.second.empty": "second box empty, not inverted",
    "cut.second.empty_inverted": "second box empty and inverted (lo = hi + 1 <= 31)",
    "cut.second.empty_inverted_past_31": "second box empty and inverted with lo = 32: avg 4 * 64 mod 256 = 0",
    "final.n_below_255": "the palette has fewer than 255 entries",
    "final.n_255": "the palette has 255 entries",
    "final.no_sample": "no sample kept: no palette",
})


def histogram(data, fmt, quality):
    """32768 bins of the kept samples and the first box (r1, r2, g1, g2, b1, b2) or None when nothing is kept."""
    ch, ri, gi, bi, ai = LAYOUT[fmt]
    data = np.asarray(data, dtype=np.uint8).reshape(-1)
    n_px = data.size // ch
    px = data[: n_px * ch].reshape(n_px, ch)[::quality].astype(np.int64)
    r, g, b = px[:, ri], px[:, gi], px[:, bi]
    a = px[:, ai] if ai is not None else np.full(r.shape, 255)
    keep = (a >= 125) & ~((r > 250) & (g > 250) & (b > 250))
    r, g, b = r[keep] >> 3, g[keep] >> 3, b[keep] >> 3
    hist = np.bincount((r << 10) | (g << 5) | b, minlength=32768).astype(np.uint32)
    if r.size == 0:
        return hist, None
    return hist, (int(r.min()), int(r.max()), int(g.min()), int(g.max()), int(b.min()), int(b.max()))


class Box:
    def __init__(self, lo, hi, hist3):
        self.lo, self.hi = list(lo), list(hi)
        sub = hist3[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] if all(l <= h for l, h in zip(lo, hi)) else np.zeros((0, 0, 0), np.uint64)
        self.count = int(sub.sum())
        self.volume = 1
        for l, h in zip(lo, hi):
            self.volume *= max(h - l + 1, 0)
        avg = []
        for axis in range(3):
            if self.count:
                s = np.arange(lo[axis], hi[axis] + 1, dtype=np.uint64) * 8 + 4
                shape = [1, 1, 1]
                shape[axis] = -1
                avg.append(int((sub * s.reshape(shape)).sum()) // self.count)
            else:
                avg.append((4 * (lo[axis] + hi[axis] + 1)) % 256)
        self.avg = tuple(avg)


def _pop(q, key):
    q.sort(key=key)   # Python's sort is stable: among equal keys the one standing last is popped first
    return q.pop()


def _t(trace, label):
    if trace is None:
        return
    if hasattr(trace, "append"):
        trace.append(label)
    else:
        trace[label] += 1


def _cut(v, hist3, trace=None):
    if v.count == 1:
        return v, None
    widths = [h - l + 1 for l, h in zip(v.lo, v.hi)]
    axis = 0 if widths[0] >= widths[1] and widths[0] >= widths[2] else (1 if widths[1] >= widths[2] else 2)
    lo, hi = v.lo[axis], v.hi[axis]
    sub = hist3[v.lo[0]:v.hi[0] + 1, v.lo[1]:v.hi[1] + 1, v.lo[2]:v.hi[2] + 1]
    slices = sub.sum(axis=tuple(a for a in range(3) if a != axis)).astype(np.int64)
    partial = {lo + k: int(x) for k, x in enumerate(np.cumsum(slices))}
    total = partial[hi]
    i = next(s for s in range(lo, hi + 1) if 2 * partial[s] > total)
    left, right = i - lo, hi - i
    d = min(hi - 1, i + right // 2) if left <= right else max(lo, i - 1 - (left + 1) // 2)
    if trace is not None:
        _t(trace, "cut.axis.%s/%s" % ("rgb"[axis], "".join(c for c, w in zip("rgb", widths) if w == max(widths))))
        if any(2 * partial[s] == total for s in range(lo, i)):
            _t(trace, "cut.median.exact_half")
        if left <= right:
            _t(trace, "cut.median.left_le_right")
            _t(trace, "cut.median.min_clipped" if hi - 1 < i + right // 2 else "cut.median.min_unclipped")
        else:
            _t(trace, "cut.median.left_gt_right")
            _t(trace, "cut.median.max_clipped" if lo > i - 1 - (left + 1) // 2 else "cut.median.max_unclipped")
        if d >= lo and partial[d] != 0:
            _t(trace, "cut.advance.none")
    while d < lo or partial[d] == 0:
        _t(trace, "cut.advance.d_below_lo" if d < lo else "cut.advance.empty_prefix")
        d += 1
    c2 = total - partial[d]
    if c2 != 0:
        _t(trace, "cut.retreat.not_entered")
    while c2 == 0 and d - 1 >= lo and partial[d - 1] != 0:
        d -= 1
        c2 = total - partial[d]
        _t(trace, "cut.retreat.stepped" if c2 == 0 else "cut.retreat.stepped_to_nonempty")
    if c2 == 0:
        _t(trace, "cut.retreat.stopped_at_lo" if d - 1 < lo else "cut.retreat.stopped_by_empty_prefix")
    hi1, lo2 = list(v.hi), list(v.lo)
    hi1[axis], lo2[axis] = d, d + 1
    if trace is not None:
        _t(trace, "cut.second.nonempty" if c2 else ("cut.second.empty" if d + 1 <= hi else
                                                     ("cut.second.empty_inverted_past_31" if d + 1 > 31 else "cut.second.empty_inverted")))
    return Box(v.lo, hi1, hist3), Box(lo2, v.hi, hist3)


def _iter(q, target, key, hist3, trace=None, phase=""):
    n, it = len(q), 0
    while it < MAX_ITERATIONS:
        if n >= target:
            _t(trace, phase + (".target_met_on_entry" if it == 0 else ".target_met_after_cut"))
            return
        it += 1
        if trace is not None:
            keys = [key(b) for b in q]
            in_order = sorted(keys)
            _t(trace, phase + (".sorted_already" if keys == in_order else ".sorted_again"))
            if len(keys) > 1 and in_order[-1] == in_order[-2]:
                _t(trace, phase + ".equal_keys_on_top")
        v = _pop(q, key)
        if v.count == 0:
            _t(trace, phase + ".count0_top")
            q.append(v)
            it += 1
            continue
        if v.count == 1:
            _t(trace, phase + (".count1_top_cuttable_below" if any(b.count > 1 for b in q) else ".count1_top_nothing_cuttable"))
        v1, v2 = _cut(v, hist3, trace)
        q.append(v1)
        if v2 is not None:
            q.append(v2)
            n += 1
    _t(trace, phase + ".iteration_cap")


def palette_from_histogram(hist, box, max_colors, trace=None):
    """trace: None, or a list / Counter that takes one label of LABELS per decision of _iter and _cut; the result is the same."""
    if box is None:
        _t(trace, "final.no_sample")
        return []
    hist3 = np.asarray(hist, dtype=np.uint64).reshape(32, 32, 32)
    key_a = lambda v: v.count                 # noqa: E731
    key_b = lambda v: v.count * v.volume      # noqa: E731
    qa = [Box((box[0], box[2], box[4]), (box[1], box[3], box[5]), hist3)]
    _iter(qa, 0.75 * max_colors, key_a, hist3, trace, "A")
    qb = []
    while qa:
        qb.append(_pop(qa, key_a))
    _iter(qb, max_colors, key_b, hist3, trace, "B")
    _t(trace, "final.n_255" if len(qb) == 255 else "final.n_below_255")
    out = []
    while qb:
        out.append(_pop(qb, key_b).avg)
    return out


def get_palette(data, fmt, quality, max_colors):
    """[(r, g, b), ...] in palette order; ValueError for a quality / max_colors the device rejects."""
    if not (1 <= quality <= 10) or not (2 <= max_colors <= 255):
        raise ValueError("quality must be 1..10 and max_colors 2..255")
    hist, box = histogram(data, fmt, quality)
    return palette_from_histogram(hist, box, max_colors)


_CSS = None


def css_colors():
    global _CSS
    if _CSS is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "css_named_colors.json")
        _CSS = [tuple(c) for c in json.load(open(path))["colors"]]
    return _CSS


def css_similar(r, g, b):
    """Nearest named colour by squared RGB distance; ties to the first name in alphabetical order."""
    best = None
    for name, cr, cg, cb in sorted(css_colors()):
        d = (cr - r) ** 2 + (cg - g) ** 2 + (cb - b) ** 2
        if best is None or d < best[0]:
            best = (d, name)
    return best[1]


def pack(palette):
    return [(r << 16) | (g << 8) | b for r, g, b in palette]
