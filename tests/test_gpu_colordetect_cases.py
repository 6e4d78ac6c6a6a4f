"""colordetect's four kernels on the directed cases of tests/colordetect_cases.py (each names the branch it was built for;
tests/test_colordetect_cases_cpu.py proves those claims): palettes, first boxes and histograms must equal the restatement's with
`==`. The MMCQ kernel gets its histograms directly (mi355_selftest_colordetect_mmcq), as frames of one pixel per sample, and as
members of the video group's launch sets; the histogram kernels get frames whose sample counts sit on both sides of every trip,
wave and block boundary, inside allocations filled with bytes that would be counted if they were read."""
import numpy as np
import pytest

import colordetect_cases as K
import colordetect_restate as R

pytestmark = pytest.mark.gpu

GREY = 0x80          # opaque mid-grey in every format: a byte read outside the plane becomes a kept sample
_CACHE = {}


def _n_cu():
    """The library does not say how many compute units the context has, and the cases do not need it: the launch geometry of
    every sample count here is the same for 3 compute units and up (tests/test_colordetect_cases_cpu.py proves it), so the content
    built for the first lane of every wave sits there on any such device."""
    return 256


def _want_hist(case):
    """(frame, restated histogram, restated box) of a histogram case: computed once, handed out read-only."""
    key = ("hist", case.name)
    if key not in _CACHE:
        f = case.frame(_n_cu())
        hist, box = R.histogram(f, case.fmt, case.quality)
        f.setflags(write=False)
        hist.setflags(write=False)
        _CACHE[key] = (f, hist, box)
    return _CACHE[key]


def _want_palette(case, mc):
    key = ("pal", case.name, mc)
    if key not in _CACHE:
        f, hist, box = _want_hist(case)
        _CACHE[key] = tuple(R.palette_from_histogram(hist, box, mc))
    return list(_CACHE[key])


class Buffer:
    """A device allocation filled with grey, planes placed inside it; `unchanged()` reads it back whole."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.host = np.full(nbytes, GREY, np.uint8)
        self.d = ctx.alloc(nbytes)
        assert self.d % 256 == 0

    def put(self, offset, plane):
        assert offset >= 64 and offset + plane.size + 64 <= self.host.size
        self.host[offset:offset + plane.size] = plane
        return self.d + offset

    def upload(self):
        self.ctx.h2d(self.d, self.host)

    def unchanged(self):
        back = np.zeros_like(self.host)
        self.ctx.d2h(back, self.d)
        return np.array_equal(back, self.host)

    def free(self):
        self.ctx.free(self.d)


def _nothing_kept(ctx, d_white):
    """A frame without a kept sample right after a call: a histogram that was not left zero would show here."""
    hist, box = ctx.colordetect_histogram_device(d_white, 64, "RGBA", 1)
    assert not hist.any() and box is None
    assert ctx.colordetect_frames_device(d_white, 64, 64, 1, "RGBA", 1, 5) == [[]]


def _white(ctx):
    d = ctx.alloc(64)
    ctx.h2d(d, np.full(64, 255, np.uint8))
    return d


# ------------------------------------------------------------------------------------------------ the MMCQ kernel

def _entry_cases(ctx, cases):
    d_white = _white(ctx)
    try:
        for case in cases:
            pal, box = ctx.selftest_colordetect_mmcq(case.bins(), case.max_colors)
            assert pal == case.expected(), (case.name, case.claims)
            assert box == case.box, (case.name, box, case.box)
            _nothing_kept(ctx, d_white)
    finally:
        ctx.free(d_white)


def test_palette_cases_through_the_entry(ctx):
    _entry_cases(ctx, [c for c in K.PALETTE_CASES if c.max_colors < 255])


def test_palette_cases_of_255_colours_through_the_entry(ctx):
    cases = [c for c in K.PALETTE_CASES if c.max_colors == 255]
    assert len(cases) == 2 and all(len(c.expected()) == 255 for c in cases)
    _entry_cases(ctx, cases)


def test_large_counts_through_the_entry(ctx):
    _entry_cases(ctx, K.LARGE_CASES)


@pytest.mark.parametrize("fmt", ["RGBA", "RGB"])
def test_palette_cases_as_frames(ctx, fmt):
    """One pixel per sample: the histogram kernel's smallest launches feed the MMCQ kernel the same bins."""
    assert len(K.FRAME_CASES) >= 60
    buf = Buffer(ctx, 4096)
    try:
        for case in K.FRAME_CASES:
            f = case.as_frame(fmt, 1)
            assert ctx.colordetect_frame(f, fmt, 1, case.max_colors) == case.expected(), (case.name, case.claims)
            buf.host[:] = GREY
            d = buf.put(64, f)
            buf.upload()
            hist, box = ctx.colordetect_histogram_device(d, f.size, fmt, 1)
            assert np.array_equal(hist, case.bins()) and box == case.box, (case.name, box)
            assert ctx.colordetect_frames_device(d, f.size, f.size, 1, fmt, 1, case.max_colors) == [case.expected()], case.name
        assert buf.unchanged()
    finally:
        buf.free()


def test_entry_refusals(ctx):
    import ctypes as C
    import mi355fx
    L, bins, pal, n, box = ctx.L, np.zeros(32768, np.uint32), np.zeros(765, np.uint8), C.c_int(0), (C.c_int * 6)()
    bins[5] = 2
    call = L.mi355_selftest_colordetect_mmcq
    assert call(None, bins.ctypes.data, 2, pal.ctypes.data, C.byref(n), box) == mi355fx.ERR_INVALID_ARG
    assert call(ctx.h, None, 2, pal.ctypes.data, C.byref(n), box) == mi355fx.ERR_INVALID_ARG
    assert call(ctx.h, bins.ctypes.data, 2, None, C.byref(n), box) == mi355fx.ERR_INVALID_ARG
    assert call(ctx.h, bins.ctypes.data, 2, pal.ctypes.data, None, box) == mi355fx.ERR_INVALID_ARG
    assert call(ctx.h, bins.ctypes.data, 2, pal.ctypes.data, C.byref(n), None) == mi355fx.ERR_INVALID_ARG
    for mc in (1, 256, 0, -1):
        assert call(ctx.h, bins.ctypes.data, mc, pal.ctypes.data, C.byref(n), box) == mi355fx.ERR_INVALID_ARG
    over = np.zeros(32768, np.uint32)
    over[0], over[32767] = 2 ** 32 - 1, 1                      # 2^32 samples: more than a frame can hold
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.selftest_colordetect_mmcq(over, 2)
    assert e.value.status == mi355fx.ERR_INVALID_ARG
    over[32767] = 0
    assert ctx.selftest_colordetect_mmcq(over, 2)[1] == (0, 0, 0, 0, 0, 0)
    want = R.palette_from_histogram(bins, (0, 0, 0, 0, 5, 5), 2)
    assert want == [(4, 4, 44), (8, 4, 44)]                    # the bin, then the inverted empty box beside it on r
    assert ctx.selftest_colordetect_mmcq(bins, 2) == (want, (0, 0, 0, 0, 5, 5))   # refused calls left no trace
    assert ctx.selftest_colordetect_mmcq(np.zeros(32768, np.uint32), 2) == ([], None)


def test_order_dependence(ctx):
    """The same list forwards and backwards on one context: what a case leaves behind would show in its neighbour."""
    cases = K.PALETTE_CASES + K.LARGE_CASES
    for order in (cases, cases[::-1]):
        for case in order:
            assert ctx.selftest_colordetect_mmcq(case.bins(), case.max_colors) == (case.expected(), case.box), case.name
            if case.samples <= K.FRAME_SAMPLES_MAX:
                assert ctx.colordetect_frame(case.as_frame("BGRA", 2), "BGRA", 2, case.max_colors) == case.expected(), case.name


# ------------------------------------------------------------------------------------------------ the histogram kernels

def _lone_hist_cases(ctx, cases):
    n_cu = _n_cu()
    biggest = max(c.data_len for c in cases)
    buf = Buffer(ctx, biggest + 256)
    d_white = _white(ctx)
    try:
        for case in cases:
            f, want, want_box = _want_hist(case)
            buf.host[:] = GREY
            d = buf.put(64 + case.misalign, f)
            buf.upload()
            assert (d % 4 == 0 and case.ch == 4) == case.word()
            hist, box = ctx.colordetect_histogram_device(d, case.data_len, case.fmt, case.quality)
            blocks, per = K.lone_geometry(case.n, n_cu)
            assert np.array_equal(hist, want), (case.name, case.claims, blocks, per, int(hist.sum()), int(want.sum()))
            assert box == want_box, (case.name, box, want_box)
            assert buf.unchanged(), case.name
        _nothing_kept(ctx, d_white)
    finally:
        ctx.free(d_white)
        buf.free()


def test_histogram_cases_up_to_one_trip(ctx):
    _lone_hist_cases(ctx, [c for c in K.HIST_CASES if c.n <= 4096])


def test_histogram_cases_second_trip_and_blocks(ctx):
    cases = [c for c in K.HIST_CASES if c.n > 4096]
    assert {c.n for c in cases} == {4097, 16384, 16385, 16385 + 1024, 32769}
    assert K.lone_geometry(16385, _n_cu()) == (2, 8193) and K.lone_geometry(32769, _n_cu())[0] == 3
    _lone_hist_cases(ctx, cases)


def test_histogram_classes_in_multi_frame_calls(ctx):
    """All content kinds of one (format, quality, length) in one call, at a pitch that keeps 4-byte formats on the dword path."""
    classes = K.hist_classes()
    assert len(classes) >= 40
    for (fmt, q, n, tail), cases in sorted(classes.items()):
        data_len = cases[0].data_len
        pitch = (data_len + 3) // 4 * 4 + 64
        buf = Buffer(ctx, 128 + pitch * len(cases))
        try:
            for k, case in enumerate(cases):
                buf.put(64 + k * pitch, _want_hist(case)[0])
            buf.upload()
            for mc in (2, 5):
                got = ctx.colordetect_frames_device(buf.d + 64, pitch, data_len, len(cases), fmt, q, mc)
                assert got == [_want_palette(case, mc) for case in cases], (fmt, q, n, tail, mc)
            assert buf.unchanged()
        finally:
            buf.free()


def test_frame_pairs_at_an_odd_pitch_take_the_byte_path(ctx):
    """Two RGBA planes at pitch data_len + 1: the second starts 1 past a dword boundary, so the batch loads bytes."""
    for n in (65, 4097, 16385):
        cases = [c for c in K.HIST_CASES if (c.fmt, c.n, c.tail, c.misalign) == ("RGBA", n, 0, 0) and c.kind in ("noise", "lead_alpha")]
        if len(cases) != 2:
            cases = [K.HistCase("RGBA", 1, n, kind, []) for kind in ("noise", "lead_alpha")]
        data_len = cases[0].data_len
        pitch = data_len + 1
        assert data_len % 4 == 0 and not cases[0].word(n_frames=2, pitch=pitch)
        buf = Buffer(ctx, 128 + 2 * pitch + 64)
        try:
            for k, case in enumerate(cases):
                buf.put(64 + k * pitch, _want_hist(case)[0])
            buf.upload()
            got = ctx.colordetect_frames_device(buf.d + 64, pitch, data_len, 2, "RGBA", cases[0].quality, 8)
            assert got == [_want_palette(case, 8) for case in cases], n
            assert buf.unchanged()
        finally:
            buf.free()


MANY_FRAMES = 320   # more than the 256 compute units of an MI355X


def test_more_frames_than_compute_units(ctx):
    """More frames than compute units in one call: one block each, though a lone frame of this length takes two."""
    cases = [K.HistCase("BGRA", 1, 16385 + 1024, kind, []) for kind in K.HIST_KINDS]
    assert K.lone_geometry(cases[0].n, 256, n_frames=MANY_FRAMES) == (1, cases[0].n) and K.lone_geometry(cases[0].n, 256)[0] == 2
    data_len = cases[0].data_len
    pitch = data_len + 4
    buf = Buffer(ctx, 128 + pitch * MANY_FRAMES)
    try:
        order = [cases[(3 * k) % len(cases)] for k in range(MANY_FRAMES)]
        for k, case in enumerate(order):
            buf.put(64 + k * pitch, _want_hist(case)[0])
        buf.upload()
        got = ctx.colordetect_frames_device(buf.d + 64, pitch, data_len, MANY_FRAMES, "BGRA", 1, 4)
        assert got == [_want_palette(case, 4) for case in order]
        assert buf.unchanged()
    finally:
        buf.free()


# ------------------------------------------------------------------------------------------------ the launch sets of the video group

def test_palette_cases_through_the_group_queue(ctx):
    """The frames of the palette cases as members of launch sets, 32 per set, formats, qualities and max_colors mixed: the job
    kernels at the same branches. Every member == its lone call == the restatement; a set is two launches."""
    import mi355fx
    cases = K.FRAME_CASES
    members = []
    for k, case in enumerate(cases):
        fmt, q = K.FORMATS[k % 5], (1, 2, 10, 3)[k % 4]
        members.append((case, fmt, q, case.as_frame(fmt, q), 64 + (k % 7 == 3)))      # every seventh plane 1 past a dword boundary
    buf = Buffer(ctx, sum(m[3].size + 192 for m in members) + 256)
    g = mi355fx.Group(0)
    try:
        at, offset = [], 0
        for case, fmt, q, f, lead in members:
            offset = (offset + 63) // 64 * 64 + lead
            at.append(buf.put(offset, f))
            offset += f.size + 64
        buf.upload()
        assert {d % 4 for d in at} == {0, 1}
        sets = 0
        for k0 in range(0, len(members), 32):
            chunk = range(k0, min(k0 + 32, len(members)))
            tickets = [g.submit_colordetect(ctx, at[k], members[k][3].size, members[k][1], members[k][2], members[k][0].max_colors) for k in chunk]
            sets += 1
            for k, t in zip(chunk, tickets):
                case, fmt, q, f, _lead = members[k]
                got = g.wait_colordetect(t)
                lone = ctx.colordetect_frames_device(at[k], f.size, f.size, 1, fmt, q, case.max_colors)[0]
                assert got == lone == case.expected(), (case.name, case.claims, fmt, q)
        assert g.colordetect_stats() == (len(members), sets, min(32, len(members)), 2 * sets)
        assert buf.unchanged()
    finally:
        g.close()
        buf.free()


def test_histogram_cases_through_the_group_queue(ctx):
    """The histogram cases with more than one trip or block, and the misaligned ones, as jobs: blocks per job come from the plan."""
    import mi355fx
    cases = [c for c in K.HIST_CASES if c.n >= 4095 or c.misalign or c.tail][:64]
    assert len(cases) == 64 and any(c.misalign for c in cases) and any(c.n == 32769 for c in cases)
    buf = Buffer(ctx, sum(c.data_len + 192 for c in cases) + 256)
    g = mi355fx.Group(0)
    try:
        at, offset = [], 0
        for c in cases:
            offset = (offset + 63) // 64 * 64 + 64 + c.misalign
            at.append(buf.put(offset, _want_hist(c)[0]))
            offset += c.data_len + 64
        buf.upload()
        for k0 in (0, 32):
            tickets = [g.submit_colordetect(ctx, at[k], cases[k].data_len, cases[k].fmt, cases[k].quality, 3 + k % 4) for k in range(k0, k0 + 32)]
            for k, t in zip(range(k0, k0 + 32), tickets):
                assert g.wait_colordetect(t) == _want_palette(cases[k], 3 + k % 4), (cases[k].name, cases[k].claims)
        assert g.colordetect_stats() == (64, 2, 32, 4)
        assert buf.unchanged()
    finally:
        g.close()
        buf.free()
