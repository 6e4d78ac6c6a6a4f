"""The directed cases of colordetect's four kernels (csrc/colordetect.hip), shared by tests/test_colordetect_cases_cpu.py (which proves
what each case claims) and tests/test_gpu_colordetect_cases.py (which holds the device to the restatement, bit for bit, on them).

  PALETTE_CASES   sparse histograms {(r5, g5, b5): count} with max_colors; every case names the labels of the traced restatement
                  (colordetect_restate.LABELS, AXIS_LABELS) and of the device's slice partition (SPLIT_LABELS) it was built for.
  LARGE_CASES     counts near 2^32: a histogram only, no frame can hold them.
  split()         a model of how cut_box deals the bins of a box to its 8 waves: the device alone has this code.
  HIST_CASES      frames for the histogram kernels, (format, quality, sample count, content), with a model of the launch geometry
                  (lone_geometry, job_plan) and of add_bin's wave situations (hist_labels) that names what each one reaches.
Not part of the product."""
from collections import Counter

import numpy as np

import colordetect_restate as R

FORMATS = ("RGB", "RGBA", "ARGB", "BGR", "BGRA")

# ------------------------------------------------------------------------------------------------ the label table

# The axis rule (widest, ties r, g, b) over every width triple: which (axis, set of widest axes) pairs exist at all. b is cut only
# when it alone is widest and g only when r is not among the widest, so "b/gb", "b/rb", "b/rgb", "g/rg" and "g/rgb" do not occur.
AXIS_LABELS = sorted({"cut.axis.%s/%s" % ("rgb"[0 if w[0] >= w[1] and w[0] >= w[2] else (1 if w[1] >= w[2] else 2)],
                                          "".join(c for c, x in zip("rgb", w) if x == max(w)))
                      for w in ((a, b, c) for a in (1, 2, 3) for b in (1, 2, 3) for c in (1, 2, 3))})

# Labels that no histogram reaches, each with its argument; the CPU test checks that none of them occurs in any case nor in an
# exhaustive sweep of small histograms. Everything else in the table must be claimed by a case.
EXEMPT = {
    "A.count0_top": "A's key is the count; the counts of the queue always sum to the frame's, which is > 0, so the largest is never 0",
    "B.count0_top": "B's key is count * volume; a box with samples has volume >= 1, so some key is > 0 and the largest is never 0",
    "A.count1_top_cuttable_below": "A is sorted by count: when the popped box has count 1 no box has more",
    "A.target_met_on_entry": "A starts with one box and its target is 0.75 * max_colors >= 1.5",
}

SPLIT_LABELS = {
    "split.parts_8": "cut axis 1 wide: each slice in 8 parts",
    "split.parts_4": "cut axis 2 wide: 4 parts",
    "split.parts_2": "cut axis 3 or 4 wide: 2 parts",
    "split.parts_1": "cut axis 5 or more wide: the slice is one part",
    "split.part_empty": "part * n1 / parts leaves a part without rows (n1 < parts)",
    "split.part_over_64_bins": "a part holds more than 64 bins: the lane loop takes a second trip",
    "split.wave_second_trip": "more than 8 (slice, part) items: the wave loop takes a second trip",
}

ALL_LABELS = sorted(set(R.LABELS) | set(AXIS_LABELS) | set(SPLIT_LABELS))


# ------------------------------------------------------------------------------------------------ cut_box's work split

def cut_axis(widths):
    return 0 if widths[0] >= widths[1] and widths[0] >= widths[2] else (1 if widths[1] >= widths[2] else 2)


def split(widths):
    """How the device sums the slices of a box of these (r, g, b) widths. Returns dict(axis, parts, items, labels): items in the order
    the waves take them, each (wave, wave_trip, slice, part, r_beg, r_end, n2, lane_trips); the bins of an item are rows
    r_beg .. r_end - 1 of the second axis (the first of the two other axes) times all n2 of the third, k = row * n2 + column, lane
    trip t taking k in [64 t, 64 t + 64)."""
    axis = cut_axis(widths)
    a1, a2 = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    w, n1, n2 = widths[axis], widths[a1], widths[a2]
    parts = 1 if w >= 8 else 8 // w
    items, labels = [], {"split.parts_%d" % parts}
    for wave in range(8):
        for trip, item in enumerate(range(wave, w * parts, 8)):
            s, part = item // parts, item % parts
            r_beg, r_end = part * n1 // parts, (part + 1) * n1 // parts
            n_bins = (r_end - r_beg) * n2
            items.append((wave, trip, s, part, r_beg, r_end, n2, (n_bins + 63) // 64))
            if r_end == r_beg:
                labels.add("split.part_empty")
            if n_bins > 64:
                labels.add("split.part_over_64_bins")
            if trip:
                labels.add("split.wave_second_trip")
    return dict(axis=axis, a1=a1, a2=a2, parts=parts, items=items, labels=labels)


def split_bins(lo, hi):
    """Every bin index the model's (slice, part, lane trip) ranges visit for the box lo .. hi, as a list (with repeats, if any)."""
    widths = [h - l + 1 for l, h in zip(lo, hi)]
    sp = split(widths)
    out = []
    for _wave, _trip, s, _part, r_beg, r_end, n2, lane_trips in sp["items"]:
        n_bins = (r_end - r_beg) * n2
        for t in range(lane_trips):
            for k in range(64 * t, min(64 * t + 64, n_bins)):
                co = [0, 0, 0]
                co[sp["axis"]] = lo[sp["axis"]] + s
                co[sp["a1"]] = lo[sp["a1"]] + r_beg + k // n2
                co[sp["a2"]] = lo[sp["a2"]] + k % n2
                out.append((co[0] << 10) | (co[1] << 5) | co[2])
    return out


# ------------------------------------------------------------------------------------------------ palette cases

class Trace(Counter):
    """The restatement's label counts of one palette."""


class PaletteCase:
    def __init__(self, name, hist, max_colors, claims):
        self.name, self.hist, self.max_colors, self.claims = name, dict(hist), max_colors, list(claims)
        self.samples = sum(self.hist.values())
        ks = sorted(self.hist)
        self.box = None if not ks else tuple(f(k[c] for k in ks) for c in range(3) for f in (min, max))
        self._want = None

    def __repr__(self):
        return "PaletteCase(%s)" % self.name

    def bins(self):
        h = np.zeros(32768, np.uint32)
        for (r, g, b), c in self.hist.items():
            h[(r << 10) | (g << 5) | b] = c
        return h

    def expected(self):
        """The restatement's palette; computed once and not handed out for writing."""
        if self._want is None:
            self._want = tuple(R.palette_from_histogram(self.bins(), self.box, self.max_colors))
        return list(self._want)

    def traced(self):
        """(palette, label counts, boxes cut) of the traced restatement."""
        t, boxes = Trace(), []
        hist3 = np.asarray(self.bins(), np.uint64).reshape(32, 32, 32)
        cut = R._cut

        def spy(v, h3, trace=None):
            if v.count != 1:
                boxes.append((tuple(v.lo), tuple(v.hi)))
            return cut(v, h3, trace)
        R._cut = spy
        try:
            pal = R.palette_from_histogram(hist3.reshape(-1), self.box, self.max_colors, t)
        finally:
            R._cut = cut
        return pal, t, boxes

    def reached(self):
        """Every label the case reaches: the restatement's and, for each box it cuts, the split model's."""
        _pal, t, boxes = self.traced()
        got = set(t)
        for lo, hi in boxes:
            got |= split([h - l + 1 for l, h in zip(lo, hi)])["labels"]
        return got

    def as_frame(self, fmt, quality=1):
        """The smallest flat plane with this histogram: one pixel per sample at 8 c + 4 (250 in bin 31, 31, 31), in bin order, quality - 1 dropped pixels
        (transparent, or white where the format has no alpha) between samples."""
        assert self.samples <= 4096, "no frame for this case"
        ch, ri, gi, bi, ai = R.LAYOUT[fmt]
        n_px = (self.samples - 1) * quality + 1 if self.samples else quality
        px = np.zeros((n_px, ch), np.uint8)
        if ai is None:
            px[:] = 255
        else:
            px[:, (ri, gi, bi)] = 128
            px[:, ai] = 124
        k = 0
        for (r, g, b) in sorted(self.hist):
            for _ in range(self.hist[(r, g, b)]):
                p = px[k * quality]
                p[ri], p[gi], p[bi] = (250, 250, 250) if (r, g, b) == (31, 31, 31) else (8 * r + 4, 8 * g + 4, 8 * b + 4)   # 252 x 3 is white
                if ai is not None:
                    p[ai] = 255
                k += 1
        return px.reshape(-1)


def _corner_box(lo, widths, counts=(1, 2)):
    """Samples at two opposite corners of the box at lo with these widths (a third, if given, at the corner that differs in r)."""
    hi = tuple(l + w - 1 for l, w in zip(lo, widths))
    h = {tuple(lo): counts[0]}
    h[hi] = h.get(hi, 0) + counts[1]
    if len(counts) > 2:
        k = (hi[0], lo[1], lo[2]) if widths[0] > 1 else (lo[0], hi[1], lo[2])
        h[k] = h.get(k, 0) + counts[2]
    return h


def _dense_box(lo, widths):
    """Every bin of the box filled, count 1 + (a mix of its coordinates) mod 5: a dropped or doubled bin moves a sum."""
    return {(lo[0] + a, lo[1] + b, lo[2] + c): 1 + (3 * a + 5 * b + 7 * c) % 5
            for a in range(widths[0]) for b in range(widths[1]) for c in range(widths[2])}


def _palette_cases():
    P = PaletteCase
    cases = [
        P("one_sample", {(30, 31, 30): 1}, 2,
          ["A.count1_top_nothing_cuttable", "A.iteration_cap", "A.sorted_already", "B.count1_top_nothing_cuttable", "B.iteration_cap",
           "B.sorted_already", "final.n_below_255"]),
        P("one_bin_twice", {(2, 2, 1): 2}, 2,
          ["cut.axis.r/rgb", "cut.median.left_le_right", "cut.median.min_clipped", "cut.advance.d_below_lo", "cut.retreat.stopped_at_lo",
           "cut.second.empty_inverted", "A.target_met_after_cut", "B.target_met_on_entry", "split.parts_8", "split.part_empty"]),
        P("one_bin_twice_at_31", {(31, 20, 5): 2}, 2, ["cut.second.empty_inverted_past_31"]),
        P("one_bin_twice_255_colours", {(7, 9, 11): 2}, 255, ["final.n_255", "A.sorted_again", "B.sorted_again"]),
        P("one_bin_twice_at_31_255_colours", {(31, 31, 30): 2}, 255, ["final.n_255", "cut.second.empty_inverted_past_31"]),
        P("a_sorted_again", {(2, 1, 3): 2}, 3, ["A.sorted_again"]),
        P("b_sorted_again", {(1, 1, 1): 2}, 4, ["B.sorted_again", "B.target_met_after_cut"]),
        P("a_equal_keys", {(31, 5, 2): 1, (5, 31, 20): 1}, 3, ["A.equal_keys_on_top"]),
        P("a_equal_keys_after_cut", {(0, 0, 0): 2, (20, 0, 0): 2}, 4, ["A.equal_keys_on_top"]),
        P("b_equal_keys", {(0, 2, 0): 1, (0, 3, 0): 1}, 3, ["B.equal_keys_on_top"]),
        P("a_equal_keys_on_g", {(0, 0, 0): 2, (0, 7, 0): 2}, 5, ["A.equal_keys_on_top", "cut.axis.g/g"]),
        P("b_stall", {(1, 0, 0): 2, (1, 20, 31): 1}, 4, ["B.count1_top_cuttable_below", "B.iteration_cap"]),
        P("b_stall_wide", {(0, 0, 0): 3, (31, 31, 31): 1}, 8, ["B.count1_top_cuttable_below", "B.iteration_cap"]),
        P("advance_empty_prefix", {(3, 0, 1): 1, (0, 3, 2): 2}, 3, ["cut.advance.empty_prefix", "cut.retreat.stopped_by_empty_prefix"]),
        P("advance_empty_prefix_far", {(0, 0, 0): 1, (20, 0, 0): 2}, 3,
          ["cut.advance.empty_prefix", "cut.retreat.stopped_by_empty_prefix", "cut.second.empty_inverted", "cut.axis.r/r"]),
        P("g_gb_exact_half", {(0, 1, 1): 1, (0, 2, 0): 1}, 2,
          ["cut.advance.none", "cut.axis.g/gb", "cut.median.exact_half", "cut.median.left_gt_right", "cut.median.max_clipped",
           "cut.retreat.not_entered", "cut.second.nonempty", "split.parts_4"]),
        P("exact_half_far", {(0, 0, 0): 2, (12, 0, 0): 1, (31, 0, 0): 1}, 2, ["cut.median.exact_half"]),
        P("b_b", {(0, 2, 0): 1, (1, 3, 2): 1}, 2, ["cut.axis.b/b", "cut.median.max_unclipped", "split.parts_2"]),
        P("g_g", {(1, 1, 1): 1, (1, 3, 2): 1}, 2, ["cut.axis.g/g"]),
        P("r_r", {(3, 3, 3): 1, (0, 3, 2): 1}, 2, ["cut.axis.r/r"]),
        P("r_rb", {(1, 0, 1): 1, (0, 0, 0): 1}, 2, ["cut.axis.r/rb"]),
        P("r_rg", {(3, 0, 1): 1, (0, 3, 3): 1}, 2, ["cut.axis.r/rg"]),
        P("r_rg_far", {(0, 0, 4): 2, (9, 9, 4): 1}, 2, ["cut.axis.r/rg"]),
        P("r_rb_far", {(0, 4, 0): 2, (9, 4, 9): 1}, 2, ["cut.axis.r/rb"]),
        P("g_gb_far", {(4, 0, 0): 2, (4, 9, 9): 1}, 2, ["cut.axis.g/gb"]),
        P("r_rgb_far", {(0, 0, 0): 2, (9, 9, 9): 1}, 2, ["cut.axis.r/rgb", "split.wave_second_trip", "split.part_over_64_bins"]),
        P("min_unclipped", {(2, 0, 2): 1, (3, 1, 0): 2}, 2, ["cut.median.min_unclipped", "cut.median.left_le_right"]),
        P("left_eq_right", {(0, 0, 0): 1, (4, 0, 0): 3, (8, 0, 0): 1}, 2, ["cut.median.left_le_right", "cut.median.min_unclipped"]),
        P("right_odd", {(0, 0, 0): 3, (7, 0, 0): 1, (4, 0, 0): 1}, 2, ["cut.median.left_le_right", "cut.median.min_unclipped"]),
        P("left_gt_right_far", {(0, 0, 0): 1, (20, 0, 0): 1, (25, 0, 0): 3}, 2, ["cut.median.left_gt_right", "cut.median.max_unclipped"]),
        P("retreat_stepped", {(5, 5, 5): 2, (20, 1, 1): 1}, 3, ["cut.retreat.stepped", "cut.second.empty", "cut.retreat.stopped_at_lo"]),
        P("retreat_to_nonempty", {(3, 1, 0): 1, (2, 0, 0): 1, (3, 2, 3): 1}, 3, ["cut.retreat.stepped_to_nonempty"]),
        P("retreat_to_nonempty_far", {(0, 0, 0): 1, (5, 0, 0): 1, (20, 0, 0): 1}, 3, ["cut.retreat.stepped", "cut.retreat.stepped_to_nonempty"]),
        P("target_three_quarters", {(0, 0, 0): 4, (1, 0, 0): 1, (31, 31, 31): 2, (30, 31, 31): 1, (16, 0, 0): 2}, 4,
          ["A.target_met_after_cut", "B.target_met_after_cut"]),
        P("r_rb_opposite", {(0, 2, 9): 1, (9, 2, 0): 1}, 3, ["cut.axis.r/rb"]),
        P("exact_half_skew", {(3, 2, 20): 1, (20, 9, 1): 1}, 2, ["cut.median.exact_half", "cut.axis.b/b"]),
        P("equal_keys_both_phases", {(2, 0, 1): 1, (2, 0, 0): 1}, 4, ["A.equal_keys_on_top", "B.equal_keys_on_top"]),
        P("three_quarters_of_four", {(5, 5, 0): 2, (31, 9, 0): 1}, 4, ["A.target_met_after_cut"]),
        P("no_sample", {}, 5, ["final.no_sample"]),
    ]
    # the device's slice partition: two or three samples at the corners of boxes of chosen widths
    for widths, lo, claims in (
            ((1, 1, 1), (4, 5, 6), ["split.parts_8", "split.part_empty"]),
            ((2, 1, 1), (4, 5, 6), ["split.parts_4", "split.part_empty"]),
            ((1, 2, 1), (4, 5, 6), ["split.parts_4", "split.part_empty"]),
            ((1, 1, 3), (4, 5, 6), ["split.parts_2", "split.part_empty"]),
            ((2, 2, 2), (30, 30, 30), ["split.parts_4", "split.part_empty"]),
            ((3, 3, 3), (0, 0, 0), ["split.parts_2"]),
            ((4, 4, 4), (28, 0, 28), ["split.parts_2"]),
            ((3, 32, 32), (29, 0, 0), ["split.parts_1", "split.part_over_64_bins", "split.wave_second_trip"]),
            ((7, 5, 1), (0, 27, 31), ["split.parts_1"]),
            ((8, 8, 8), (8, 8, 8), ["split.parts_1"]),
            ((9, 1, 1), (23, 0, 0), ["split.parts_1", "split.wave_second_trip"]),
            ((9, 9, 8), (0, 0, 0), ["split.parts_1", "split.wave_second_trip", "split.part_over_64_bins"]),
            ((32, 32, 32), (0, 0, 0), ["split.parts_1", "split.wave_second_trip", "split.part_over_64_bins"])):
        name = "corners_%dx%dx%d" % widths
        cases.append(P(name, _corner_box(lo, widths, (1, 2)), 2, claims))
        cases.append(P(name + "_three", _corner_box(lo, widths, (2, 1, 2)), 4, claims))
    # ... and every bin of such a box filled (more than 16 samples: these reach the MMCQ kernel as histograms only)
    for widths, lo, mc, claims in (
            ((3, 3, 3), (7, 7, 7), 6, ["split.parts_2"]),
            ((2, 2, 2), (0, 30, 0), 4, ["split.parts_4", "split.part_empty"]),
            ((4, 3, 2), (0, 0, 0), 8, ["split.parts_2"]),
            ((3, 32, 32), (29, 0, 0), 8, ["split.parts_1", "split.part_over_64_bins", "split.wave_second_trip"]),
            ((8, 8, 8), (8, 8, 8), 8, ["split.parts_1"]),
            ((9, 9, 8), (0, 0, 0), 8, ["split.part_over_64_bins", "split.wave_second_trip"]),
            ((32, 32, 32), (0, 0, 0), 16, ["split.part_over_64_bins", "split.wave_second_trip"])):
        cases.append(P("dense_%dx%dx%d" % widths, _dense_box(lo, widths), mc, claims))
    assert len({c.name for c in cases}) == len(cases)
    return cases


PALETTE_CASES = _palette_cases()
FRAME_SAMPLES_MAX = 16
FRAME_CASES = [c for c in PALETTE_CASES if c.samples <= FRAME_SAMPLES_MAX]   # these also run as frames, through both histogram kernels

# counts near 2^32: the 64-bit paths (2 * p > total, count * volume, the colour sums)
LARGE_CASES = [PaletteCase("large_%s_%d" % (name, mc), hist, mc, [])
               for name, hist in (("one_bin", {(13, 17, 29): 2 ** 32 - 1}),
                                  ("two_bins", {(3, 4, 5): 2 ** 31, (3, 4, 9): 2 ** 31 - 1}),
                                  ("two_corners", {(0, 0, 0): 2 ** 31 - 1, (31, 31, 31): 2 ** 31 - 1}))
               for mc in (2, 8)]


# ------------------------------------------------------------------------------------------------ histogram cases

HIST_THREADS, HIST_UNROLL, SAMPLES_PER_BLOCK_MIN = 1024, 4, 16384
HIST_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16384, 16385, 16385 + 1024, 32769)
HIST_KINDS = ("solid", "alt2", "lead_alpha", "lead_white", "noise")
MAX_FRAME_PIXELS = 32769

HIST_LABELS = {
    "add_bin.all_same": "a full wave whose 64 lanes hold one bin: one atomic with the popcount",
    "add_bin.lead_dropped": "the lead lane holds no bin (dropped sample) while other lanes do",
    "add_bin.lead_mixed": "the lead lane holds a bin and lanes with other bins add singly beside it",
    "add_bin.partial_wave": "a wave with lanes on both sides of the end of the block's range",
    "hist.unroll_partial": "a trip of the 4-sample unroll with fewer than 4096 samples left",
    "hist.second_trip": "a block with more than 4096 samples: a second trip",
    "hist.blocks_2plus": "two or more blocks for one frame",
    "hist.block_boundary_mid_wave": "samples_per_block is no multiple of 64",
    "path.dword": "4-byte pixels at a 4-byte aligned address: dword loads",
    "path.byte": "byte loads",
}


def samples_of(data_len, ch, quality):
    return (data_len // ch + quality - 1) // quality


def lone_geometry(n, n_cu, n_frames=1):
    """(blocks per frame, samples per block) of colordetect_hist_kernel for frames of n samples."""
    blocks = max(1, min(-(-n_cu // n_frames), -(-n // SAMPLES_PER_BLOCK_MIN)))
    return blocks, -(-n // blocks)


def job_plan(n_cu, ns):
    """(first_block, blocks, samples_per_block, total) of a launch set's jobs, as DESIGN §4.8 "Plan" states it."""
    total_samples, with_samples = sum(ns), sum(1 for n in ns if n)
    spare = max(n_cu - with_samples, 0)
    first, blocks, per, nxt = [], [], [], 0
    for n in ns:
        b = p = 0
        if n:
            b = min(1 + n * spare // total_samples, -(-n // SAMPLES_PER_BLOCK_MIN))
            p = -(-n // b)
            b = -(-n // p)
        first.append(nxt)
        blocks.append(b)
        per.append(p)
        nxt += b
    return first, blocks, per, nxt


def block_ranges(n, blocks, per_block):
    return [(b * per_block, min((b + 1) * per_block, n)) for b in range(blocks)]


def wave_walk(sample_bins, blocks, per_block):
    """The histogram and the wave situations of hist_accumulate + add_bin over sample_bins (int64, -1: dropped), wave by wave as
    the device forms them: a model of the kernel's counting, to be compared with a plain bincount."""
    n = len(sample_bins)
    hist = np.zeros(32768, np.int64)
    labels = set()
    if blocks > 1:
        labels.add("hist.blocks_2plus")
        if per_block % 64:
            labels.add("hist.block_boundary_mid_wave")
    span = HIST_THREADS * HIST_UNROLL
    for s0, s1 in block_ranges(n, blocks, per_block):
        for trip, s in enumerate(range(s0, s1, span)):
            if trip:
                labels.add("hist.second_trip")
            if s1 - s < span:
                labels.add("hist.unroll_partial")
            for w0 in range(s, s + span, 64):          # a wave's 64 lanes of one unrolled step are 64 consecutive samples
                lanes = np.full(64, -1, np.int64)
                m = max(0, min(64, s1 - w0))
                lanes[:m] = sample_bins[w0:w0 + m]
                if 0 < m < 64:
                    labels.add("add_bin.partial_wave")
                lead = lanes[0]
                same = lanes == lead
                if lead >= 0:
                    hist[lead] += int(same.sum())
                    if m == 64 and same.all():
                        labels.add("add_bin.all_same")
                    elif (lanes[~same] >= 0).any():
                        labels.add("add_bin.lead_mixed")
                elif (lanes >= 0).any():
                    labels.add("add_bin.lead_dropped")
                rest = lanes[~same]
                np.add.at(hist, rest[rest >= 0], 1)
    return hist, labels


SOLID, OTHER = (84, 124, 204), (20, 250, 36)


class HistCase:
    """n samples of one content kind in one format at one quality; `tail` bytes past the last whole pixel, the plane `misalign` bytes
    past a 4-byte boundary."""

    def __init__(self, fmt, quality, n, kind, claims, tail=0, misalign=0):
        self.fmt, self.quality, self.n, self.kind, self.claims, self.tail, self.misalign = fmt, quality, n, kind, list(claims), tail, misalign
        self.ch = R.LAYOUT[fmt][0]
        self.pixels = (n - 1) * quality + 1
        assert self.pixels <= MAX_FRAME_PIXELS and tail < self.ch
        self.data_len = self.pixels * self.ch + tail
        self.name = "%s-q%d-n%d-%s%s%s" % (fmt, quality, n, kind, "-tail%d" % tail if tail else "", "-at%d" % misalign if misalign else "")

    def __repr__(self):
        return "HistCase(%s)" % self.name

    def word(self, n_frames=1, pitch=None):
        return self.ch == 4 and self.misalign % 4 == 0 and (n_frames == 1 or (pitch if pitch is not None else self.data_len) % 4 == 0)

    def frame(self, n_cu=256):
        """The plane. Pixels between samples and the tail bytes hold mid-grey, opaque: sampled by mistake they would be kept."""
        ch, ri, gi, bi, ai = R.LAYOUT[self.fmt]
        blocks, per = lone_geometry(self.n, n_cu)
        k = np.arange(self.n)
        lead = (k - (k // per) * per) % 64 == 0        # the first lane of every wave, in every block
        rgb = np.empty((self.n, 3), np.uint8)
        alpha = np.full(self.n, 255, np.uint8)
        rgb[:] = SOLID
        if self.kind == "alt2":
            rgb[1::2] = OTHER
        elif self.kind == "lead_alpha":
            assert ai is not None
            alpha[lead] = 124
        elif self.kind == "lead_white":
            rgb[lead] = (251, 251, 251)
        elif self.kind == "noise":
            rng = np.random.default_rng(self.n * 10 + self.quality)
            rgb = rng.integers(0, 256, (self.n, 3), dtype=np.uint8)
            alpha = rng.integers(100, 150, self.n, dtype=np.uint8)
        else:
            assert self.kind == "solid"
        px = np.full((self.pixels, ch), 128, np.uint8)
        s = px[::self.quality]
        s[:, ri], s[:, gi], s[:, bi] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
        if ai is not None:
            s[:, ai] = alpha
        return np.concatenate([px.reshape(-1), np.full(self.tail, 128, np.uint8)])

    def sample_bins(self, n_cu=256):
        """The bin of every sample in order, -1 where it is dropped: what the kernel's lanes hold."""
        ch, ri, gi, bi, ai = R.LAYOUT[self.fmt]
        f = self.frame(n_cu)
        px = f[: (f.size // ch) * ch].reshape(-1, ch)[::self.quality].astype(np.int64)
        a = px[:, ai] if ai is not None else np.full(len(px), 255)
        keep = (a >= 125) & ~((px[:, ri] > 250) & (px[:, gi] > 250) & (px[:, bi] > 250))
        return np.where(keep, ((px[:, ri] >> 3) << 10) | ((px[:, gi] >> 3) << 5) | (px[:, bi] >> 3), -1)

    def reached(self, n_cu=256):
        blocks, per = lone_geometry(self.n, n_cu)
        _hist, labels = wave_walk(self.sample_bins(n_cu), blocks, per)
        return labels | {"path.dword" if self.word() else "path.byte"}


def _hist_cases():
    cases = []
    with_alpha = (("RGBA", 1), ("BGRA", 2), ("ARGB", 10), ("ARGB", 1), ("RGBA", 10))
    others = (("RGB", 1), ("BGR", 2), ("RGB", 10), ("BGR", 1), ("RGB", 2), ("BGR", 10))
    for i, n in enumerate(HIST_COUNTS):
        for fmt, q in (with_alpha[i % len(with_alpha)], others[i % len(others)]):   # two (format, quality) classes per count
            while (n - 1) * q + 1 > MAX_FRAME_PIXELS:
                q = {10: 2, 2: 1}[q]
            geo = []
            if n > 4096:
                geo.append("hist.second_trip")
            if n > SAMPLES_PER_BLOCK_MIN:
                geo.append("hist.blocks_2plus")
            if n > SAMPLES_PER_BLOCK_MIN:
                geo.append("hist.block_boundary_mid_wave")
            if n % 64:
                geo.append("add_bin.partial_wave")
            if n % 4096:
                geo.append("hist.unroll_partial")
            geo.append("path.dword" if R.LAYOUT[fmt][0] == 4 else "path.byte")
            for kind in HIST_KINDS:
                if kind == "lead_alpha" and R.LAYOUT[fmt][4] is None:
                    continue
                own = []
                if n >= (1023 if kind == "noise" else 64):
                    own = {"solid": ["add_bin.all_same"], "alt2": ["add_bin.lead_mixed"], "lead_alpha": ["add_bin.lead_dropped"],
                           "lead_white": ["add_bin.lead_dropped"], "noise": ["add_bin.lead_mixed"]}[kind]
                cases.append(HistCase(fmt, q, n, kind, geo + own))
    # the byte path for 4-byte pixels, and planes that end inside a pixel
    for mis in (1, 2, 3):
        cases.append(HistCase("RGBA", 1, 4097, "noise", ["path.byte", "hist.second_trip", "add_bin.lead_mixed"], misalign=mis))
        cases.append(HistCase("BGRA", 2, 65, "lead_alpha", ["path.byte", "add_bin.lead_dropped", "add_bin.partial_wave"], misalign=mis))
    for fmt in FORMATS:
        for tail in range(1, R.LAYOUT[fmt][0]):
            cases.append(HistCase(fmt, 1, 1025, "alt2", ["add_bin.lead_mixed", "add_bin.partial_wave"], tail=tail))
            cases.append(HistCase(fmt, 10, 63, "noise", ["add_bin.partial_wave"], tail=tail))
    assert len({c.name for c in cases}) == len(cases)
    return cases


HIST_CASES = _hist_cases()


def hist_classes():
    """The aligned cases grouped by (format, quality, sample count): one multi-frame call each."""
    out = {}
    for c in HIST_CASES:
        if not c.misalign:
            out.setdefault((c.fmt, c.quality, c.n, c.tail), []).append(c)
    return out
