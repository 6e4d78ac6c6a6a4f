"""GPU tests for the hsvfilter queue of the dispatcher (mi355_group_submit_hsvfilter / _wait_hsvfilter): the frames of INDEPENDENT
hsvfilter instances (one buffer per call and element, settings snapshotted per buffer: video/hsv/src/hsvfilter/imp.rs:85, :323-376)
filtered in place in shared launch sets - at most two launches over a job table: hsvfilter_jobs_kernel (four pixels per lane, one
v_perm_b32 into the canonical byte order and one out of it) for the frames of the lone entry's flat, rgb24 and rowpad classes with
FAST settings, hsvfilter_rows_jobs_kernel (one pixel per lane, literal where the settings need it) for the rest. Members differ in
size, stride, alignment, format and settings.

The bar is `==` on the WHOLE arena against (a) Context.hsvfilter_frames_device on a second arena prepared alike and (b)
oracle.hsvfilter on the host image. Every arena starts as a sentinel pattern with the frames' pixels drawn into it and holds the
bytes before an offset start, the row padding and at least 64 bytes behind each frame (none where a test puts frames back to back),
so an equal arena also proves that nothing outside the pixels was written."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FMT4 = ("RGBx", "xRGB", "BGRx", "xBGR", "RGBA", "ARGB", "BGRA", "ABGR")
FMTS = FMT4 + ("RGB", "BGR")
IDENT = (1.0, 0.0, 1.0, 0.0)
SV = (1.25, -0.05, 0.8, 0.1)
# every FAST variant: zero / positive / negative / wide positive / wide negative shift x identity or not
FAST_SETTINGS = [(h,) + sv for h in (0.0, 90.0, -90.0, 400.0, -4194304.0) for sv in (IDENT, SV)]
GENERIC = (1.0e7,) + SV          # beyond 2^22: the literal arithmetic, fmodf of a large operand


class Arena:
    """Two device allocations prepared alike - the group filters in one, the lone entry in the other - and the host image the oracle
    filters. Frames are carved from the same offsets of all three; `upload` sends the image once every frame has drawn its pixels."""

    def __init__(self, c, nbytes):
        self.c, self.n, self.top = c, nbytes, 0
        self.init = ((np.arange(nbytes, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
        self.exp = None
        self.dg, self.dl = c.alloc(nbytes), c.alloc(nbytes)
        assert self.dg % 16 == 0 and self.dl % 16 == 0

    def carve(self, nbytes, lead=0, tail=64):
        """`nbytes` at a 16-byte aligned offset + lead, `tail` sentinel bytes behind it."""
        off = (self.top + 15) // 16 * 16 + lead
        self.top = off + nbytes + tail
        assert self.top <= self.n, "arena too small"
        return off

    def upload(self):
        self.exp = self.init.copy()
        self.c.h2d(self.dg, self.init)
        self.c.h2d(self.dl, self.init)

    def read(self):
        got_g, got_l = np.zeros(self.n, np.uint8), np.zeros(self.n, np.uint8)
        self.c.synchronize()
        self.c.d2h(got_g, self.dg)
        self.c.d2h(got_l, self.dl)
        return got_g, got_l

    def check(self):
        got_g, got_l = self.read()
        assert (got_g == got_l).all(), "group != lone entry at bytes %s" % np.flatnonzero(got_g != got_l)[:8]
        assert (got_g == self.exp).all(), "group != oracle at bytes %s" % np.flatnonzero(got_g != self.exp)[:8]
        return got_g

    def free(self):
        self.c.free(self.dg)
        self.c.free(self.dl)


class Frame:
    """One member's frame in the arena: `at` places it inside another frame's bytes instead of carving."""

    def __init__(self, c, arena, w, h, fmt, st, seed=1, pad=0, lead=0, tail=64, at=None, pixels=None):
        from mi355fx import FMT_LAYOUT
        self.c, self.arena, self.w, self.h, self.fmt, self.st = c, arena, w, h, fmt, tuple(float(v) for v in st)
        self.ps, self.first, self.bgr = FMT_LAYOUT[fmt]
        self.stride = w * self.ps + pad
        self.nbytes = (h - 1) * self.stride + w * self.ps if w > 0 and h > 0 else 0
        if at is not None:
            self.off = at
            return
        self.off = arena.carve(self.nbytes, lead=lead, tail=tail)
        rng = np.random.default_rng(seed)
        for r in range(h if w > 0 else 0):
            row = arena.init[self.off + r * self.stride: self.off + r * self.stride + w * self.ps]
            row[:] = rng.integers(0, 256, row.size, dtype=np.uint8) if pixels is None else pixels[r * w * self.ps: (r + 1) * w * self.ps]

    def submit(self, g, c=None, st=None):
        return g.submit_hsvfilter(c or self.c, self.arena.dg + self.off, self.w, self.h, self.stride, self.fmt, st or self.st)

    def lone(self, c=None, st=None):
        (c or self.c).hsvfilter_frames_device(self.arena.dl + self.off, 1, 0, self.w, self.h, self.stride, self.fmt, st or self.st)
        (c or self.c).synchronize()

    def expect(self, oracle, st=None):
        """The oracle's filter over the frame's rows in the arena's host image (the last row ends with its pixels)."""
        if not self.nbytes:
            return
        e, lb = self.arena.exp, self.w * self.ps
        if self.h > 1:
            oracle.hsvfilter(e[self.off: self.off + (self.h - 1) * self.stride], self.w, self.stride, self.ps, self.first, bool(self.bgr), st or self.st)
        last = self.off + (self.h - 1) * self.stride
        oracle.hsvfilter(e[last: last + lb], self.w, lb, self.ps, self.first, bool(self.bgr), st or self.st)

    def pixels(self, image):
        """The frame's pixel bytes in an arena image, [h, w, ps]."""
        rows = [image[self.off + r * self.stride: self.off + r * self.stride + self.w * self.ps] for r in range(self.h)]
        return np.stack(rows).reshape(self.h, self.w, self.ps)


def _finish(oracle, arena, runs):
    """Lone entry + oracle for every (frame[, context[, settings]]) in the order given, then the whole-arena comparison."""
    for run in runs:
        f = run[0] if isinstance(run, tuple) else run
        c = run[1] if isinstance(run, tuple) and len(run) > 1 else None
        st = run[2] if isinstance(run, tuple) and len(run) > 2 else None
        f.lone(c, st)
        f.expect(oracle, st)
    got = arena.check()
    assert (got != arena.init).any()
    return got


def test_unlike_members_one_set_one_launch(ctx, oracle):
    """Thirty vector-class members: every format at three of the five sizes - one group, 256 groups (a block's lanes), 257 - and every
    FAST variant, back to back in one allocation: an overrun lands in a neighbour."""
    import mi355fx
    sizes = [(4, 1), (64, 4), (256, 4), (257, 4), (8, 2)]
    settings = FAST_SETTINGS + [(360.0,) + IDENT, (-360.0,) + SV]
    arena = Arena(ctx, 256 * 1024)
    frames = []
    for k, fmt in enumerate(FMTS):
        for j in range(3):
            w, h = sizes[(k + j) % 5]
            frames.append(Frame(ctx, arena, w, h, fmt, settings[len(frames) % len(settings)], seed=len(frames) + 1, tail=0))
    arena.upload()
    g = mi355fx.Group(0)
    try:
        assert len(frames) == 30 and {(f.w, f.h) for f in frames} == set(sizes)
        assert all(f.off % 16 == 0 for f in frames)
        assert all(b.off - (a.off + a.nbytes) < 16 for a, b in zip(frames, frames[1:]))      # back to back (to the next 16-byte mark)
        rc, n_sets, plan = mi355fx.selftest_hsvfilter_set_plan([(arena.dg + f.off, f.w, f.h, f.stride, f.fmt, f.st) for f in frames])
        assert rc == 0 and n_sets == 1 and all(p["launch"] == 1 for p in plan)
        assert {p["variant"] for p in plan} == {0, 1, 2, 4, 5, 6, 8, 9, 12, 13}
        tk = [f.submit(g) for f in frames]
        assert g.hsvfilter_stats() == (0, 0, 0, 0)                                            # nothing goes out before a wait or a full set
        for t in reversed(tk):
            g.wait_hsvfilter(t)
        assert g.hsvfilter_stats() == (30, 1, 30, 1)
        _finish(oracle, arena, frames)
    finally:
        g.close()
        arena.free()


def test_the_literal_launch(ctx, oracle):
    import mi355fx
    arena = Arena(ctx, 64 * 1024)
    generic = mi355fx.Context(0)
    generic.set_flag(mi355fx.FLAG_FORCE_GENERIC, 1)
    hue90 = (90.0,) + SV
    literal = [
        Frame(ctx, arena, 1, 1, "RGBx", hue90, seed=1),                              # 4 bytes: no whole group
        Frame(ctx, arena, 3, 5, "RGB", hue90, seed=2),                               # 45 bytes
        Frame(ctx, arena, 5, 3, "ARGB", (-90.0,) + IDENT, seed=3),                   # 60 bytes
        Frame(ctx, arena, 16, 3, "BGR", hue90, seed=4, lead=1),                      # bases off the grid
        Frame(ctx, arena, 16, 3, "BGRA", hue90, seed=5, lead=3),
        Frame(ctx, arena, 16, 3, "xBGR", (400.0,) + SV, seed=6, lead=4),             # a 4-byte frame at base + 4; a wide shift, one pixel per lane
        Frame(ctx, arena, 16, 3, "RGBA", hue90, seed=7, pad=4),                      # padded strides that are no multiple of 16
        Frame(ctx, arena, 37, 3, "RGB", (0.0,) + SV, seed=8, pad=5),
        Frame(ctx, arena, 64, 5, "RGBx", (float("nan"),) + IDENT, seed=9),           # aligned and packed, but GENERIC settings
        Frame(ctx, arena, 64, 5, "BGR", (float("inf"),) + SV, seed=10),
        Frame(ctx, arena, 64, 5, "xRGB", (float("-inf"),) + SV, seed=11),
        Frame(ctx, arena, 64, 5, "ABGR", (5e-31,) + SV, seed=12),
        Frame(generic, arena, 64, 48, "BGRx", hue90, seed=14),                       # a force-generic member: 12 blocks
    ]
    vector = [Frame(ctx, arena, 64, 48, "RGBx", hue90, seed=15),                     # aligned and packed
              Frame(ctx, arena, 13, 7, "xRGB", hue90, seed=16, pad=12),              # the rowpad class: stride 64, a one-pixel group at each row's end
              Frame(ctx, arena, 6, 3, "BGRA", (-400.0,) + SV, seed=17, pad=8)]       # ... stride 32, a two-pixel group
    empty = [Frame(ctx, arena, 0, 3, "RGBx", hue90), Frame(ctx, arena, 16, 0, "RGB", hue90), Frame(ctx, arena, 0, 0, "BGRA", hue90)]
    arena.upload()
    g = mi355fx.Group(0)
    try:
        assert literal[3].off % 4 == 1 and literal[4].off % 16 == 3 and literal[5].off % 16 == 4
        assert vector[1].stride == 64 and vector[2].stride == 32
        plan = mi355fx.selftest_hsvfilter_set_plan([(arena.dg + f.off, f.w, f.h, f.stride, f.fmt, f.st, int(f.c is generic)) for f in literal + vector])[2]
        assert [p["launch"] for p in plan] == [2] * len(literal) + [1] * len(vector)
        runs = []
        tk = [f.submit(g) for f in literal]
        for t in tk:
            g.wait_hsvfilter(t)
        runs += [(f, f.c) for f in literal]
        assert g.hsvfilter_stats() == (13, 1, 13, 1)                                 # literal jobs alone: one launch
        both = literal[:4] + vector + literal[4:]
        tk = [f.submit(g) for f in both]                                             # the literal frames once more: filtered twice
        for t in reversed(tk):
            g.wait_hsvfilter(t)
        runs += [(f, f.c) for f in both]
        assert g.hsvfilter_stats() == (29, 2, 16, 3)                                 # both classes: two launches
        tk = [f.submit(g) for f in empty]
        tk.append(g.submit_hsvfilter(ctx, None, 0, 7, 0, "RGBx", hue90))             # a null pointer is fine without a pixel
        tk.append(g.submit_hsvfilter(ctx, None, 16, 0, 64, "BGR", hue90))
        for t in tk:
            g.wait_hsvfilter(t)
        assert g.hsvfilter_stats() == (34, 3, 16, 3)                                 # no frame with a pixel: no launch
        _finish(oracle, arena, runs)
    finally:
        g.close()
        generic.close()
        arena.free()


def test_the_x_or_alpha_byte_comes_back_unchanged(ctx, oracle):
    """Random fourth bytes in all eight 4-byte formats, through the vector launch (packed and rowpad) and the literal one."""
    import mi355fx
    arena = Arena(ctx, 64 * 1024)
    frames = []
    for k, fmt in enumerate(FMT4):
        st = FAST_SETTINGS[(3 * k + 1) % len(FAST_SETTINGS)]
        frames.append(Frame(ctx, arena, 32, 6, fmt, st, seed=30 + k))                        # vector, packed
        frames.append(Frame(ctx, arena, 7, 5, fmt, st, seed=40 + k, pad=4))                  # vector, rowpad: stride 32, a three-pixel group
        frames.append(Frame(ctx, arena, 9, 5, fmt, GENERIC if k % 2 else st, seed=50 + k, lead=4))   # literal
    arena.upload()
    g = mi355fx.Group(0)
    try:
        tk = [f.submit(g) for f in frames]
        for t in tk:
            g.wait_hsvfilter(t)
        assert g.hsvfilter_stats() == (24, 1, 24, 2)
        got = _finish(oracle, arena, frames)
        for f in frames:
            x = 0 if f.first else 3
            before, after = f.pixels(arena.init), f.pixels(got)
            assert (after[:, :, x] == before[:, :, x]).all(), f.fmt
            assert len(np.unique(before[:, :, x])) > 8
    finally:
        g.close()
        arena.free()


def test_all_colours_every_variant_one_rendezvous(ctx, oracle, synth):
    """All 2^24 colours through each of the ten FAST variants and the literal arithmetic, the ten formats rotating over the eleven
    members, in ONE launch set of two launches - the squeezed plan: the vector jobs want 10 x 8192 blocks of the 256 x 64 there are,
    so every job runs its stride loop many times. Pins that the canonical <0, 1, 2, 3> arithmetic plus the two perms is the
    per-format instance the lone entry picks, colour by colour."""
    import mi355fx
    allc = synth.allcolors()
    n_px = 1 << 24
    members = []
    for k, st in enumerate(FAST_SETTINGS + [GENERIC]):
        fmt = FMTS[k % len(FMTS)]
        ps, first, _ = mi355fx.FMT_LAYOUT[fmt]
        px = allc.reshape(n_px, 4)
        host = np.ascontiguousarray(px[:, :3] if ps == 3 else (np.roll(px, 1, axis=1) if first else px)).reshape(-1)
        dg, dl = ctx.alloc(host.nbytes), ctx.alloc(host.nbytes)
        ctx.h2d(dg, host)
        ctx.h2d(dl, host)
        members.append((fmt, st, host, dg, dl))
    g = mi355fx.Group(0)
    g.set_hsvfilter_rendezvous(len(members), 2_000_000)
    try:
        plan = mi355fx.selftest_hsvfilter_set_plan([(dg, 4096, 4096, 4096 * mi355fx.FMT_LAYOUT[fmt][0], fmt, st) for fmt, st, _, dg, _ in members], n_cu=256)[2]
        assert [p["variant"] for p in plan] == [4, 0, 5, 1, 6, 2, 12, 8, 13, 9, -1] and [p["launch"] for p in plan] == [1] * 10 + [2]
        assert all(p["blocks"] < -(-p["units"] // 512) for p in plan[:10])                   # squeezed
        tk = [g.submit_hsvfilter(ctx, dg, 4096, 4096, 4096 * mi355fx.FMT_LAYOUT[fmt][0], fmt, st) for fmt, st, _, dg, _ in members]
        assert g.hsvfilter_stats() == (11, 1, 11, 2)                                         # the eleventh submit completed the rendezvous
        for t in tk:
            g.wait_hsvfilter(t)
        for fmt, st, host, dg, dl in members:
            ps, first, bgr = mi355fx.FMT_LAYOUT[fmt]
            ctx.hsvfilter_frames_device(dl, 1, 0, 4096, 4096, 4096 * ps, fmt, st)
            got_g, got_l = np.empty_like(host), np.empty_like(host)
            ctx.synchronize()
            ctx.d2h(got_g, dg)
            ctx.d2h(got_l, dl)
            exp = host.copy()
            oracle.hsvfilter(exp, 4096, 4096 * ps, ps, first, bool(bgr), st, nthreads=16)
            assert (got_g == got_l).all(), (fmt, st, np.flatnonzero(got_g != got_l)[:8])
            assert (got_g == exp).all(), (fmt, st, np.flatnonzero(got_g != exp)[:8])
    finally:
        g.close()
        for _, _, _, dg, dl in members:
            ctx.free(dg)
            ctx.free(dl)


def test_overlapping_frames_come_out_in_submission_order(ctx, oracle):
    import mi355fx
    arena = Arena(ctx, 64 * 1024)
    a = Frame(ctx, arena, 64, 16, "RGBA", (90.0,) + SV, seed=60)
    b = Frame(ctx, arena, 64, 16, "BGR", (-90.0,) + IDENT, seed=61)
    c = Frame(ctx, arena, 33, 5, "xRGB", (30.0,) + SV, seed=62, pad=4)
    inside = Frame(ctx, arena, 8, 4, "RGBA", (200.0,) + SV, pad=(64 - 8) * 4, at=a.off + 3 * a.stride + 5 * 4)   # a sub-rectangle of `a`: rows 3-6, columns 5-12
    arena.upload()
    g = mi355fx.Group(0)
    try:
        second = (45.0,) + IDENT
        t1 = a.submit(g)
        t2 = b.submit(g)
        assert g.hsvfilter_stats() == (0, 0, 0, 0)
        t3 = a.submit(g, st=second)                  # the same bytes: what was pending goes out first
        assert g.hsvfilter_stats() == (2, 1, 2, 1)
        t4 = c.submit(g)                             # disjoint frames of one allocation share the set
        t5 = inside.submit(g)                        # inside the pending second run of `a`
        assert g.hsvfilter_stats() == (4, 2, 2, 3)   # {a', c}: a vector and a literal job
        for t in (t5, t4, t3, t2, t1):
            g.wait_hsvfilter(t)
        assert g.hsvfilter_stats() == (5, 3, 2, 4)
        got = _finish(oracle, arena, [a, b, (a, None, second), c, inside])
        # the order is visible: the other order gives other bytes
        other = arena.init.copy()
        arena.exp = other
        for f, st in ((a, second), (a, None)):
            f.expect(oracle, st)
        assert (a.pixels(other) != a.pixels(got)).any()
    finally:
        g.close()
        arena.free()


def test_more_than_a_set(ctx, oracle):
    import mi355fx
    arena = Arena(ctx, 16 * 1024)
    frames = [Frame(ctx, arena, 4 + k % 3, 1 + k % 2, FMTS[k % 10], FAST_SETTINGS[k % 10], seed=70 + k) for k in range(33)]
    arena.upload()
    g = mi355fx.Group(0)
    try:
        tk = [f.submit(g) for f in frames]
        assert g.hsvfilter_stats()[:3] == (32, 1, 32)        # the 32nd submit filled a set
        for t in tk:
            g.wait_hsvfilter(t)
        assert g.hsvfilter_stats()[:3] == (33, 2, 32)
        _finish(oracle, arena, frames)
    finally:
        g.close()
        arena.free()


def test_a_frame_is_filtered_after_what_its_stream_held(ctx, oracle, synth):
    """Six lone hsvfilter launches in place, queued asynchronously on the member's stream, then the group submit on the same bytes at
    once, no host wait between: the set runs behind them on the queue's own stream."""
    import mi355fx
    w, h = 1920, 1080
    src = synth.smooth_frame(w, h).reshape(-1)
    hue90, mine = (90.0,) + IDENT, (-35.0,) + SV
    arena = Arena(ctx, w * h * 4 + 128)
    f = Frame(ctx, arena, w, h, "RGBA", mine, pixels=src)
    arena.upload()
    g = mi355fx.Group(0)
    try:
        for _ in range(6):
            ctx.hsvfilter_frames_device(arena.dg + f.off, 1, 0, w, h, w * 4, "RGBA", hue90)
        t = f.submit(g)
        g.wait_hsvfilter(t)
        _finish(oracle, arena, [(f, None, hue90)] * 6 + [f])
    finally:
        g.close()
        arena.free()


def test_protocol(ctx, oracle, synth):
    import mi355fx
    cube = oracle.Cube.parse(synth.cube_text_3d(17))
    sc, of = cube.domain
    ctx.colorlut_load(cube.is3d, cube.size, cube.table, sc, of)
    arena = Arena(ctx, 128 * 1024)
    hue90 = (90.0,) + SV
    frames = [Frame(ctx, arena, 64, 48, FMT4[k], hue90, seed=80 + k) for k in range(4)] + [Frame(ctx, arena, 33, 21, "RGB", GENERIC, seed=85)]
    det_src, det_dst = Frame(ctx, arena, 64, 48, "RGBx", hue90, seed=86), Frame(ctx, arena, 64, 48, "RGBA", hue90, seed=87)
    chain_src, chain_dst = Frame(ctx, arena, 64, 48, "RGBA", hue90, seed=88), Frame(ctx, arena, 64, 48, "RGBA", hue90, seed=89)
    arena.upload()
    g = mi355fx.Group(0)
    try:
        f = frames[0]
        d = arena.dg + f.off
        bad = [
            lambda: g.submit_hsvfilter(ctx, d, 64, 48, 512, "RGBA64_LE", hue90),       # not one of the ten 8-bit formats
            lambda: g.submit_hsvfilter(ctx, d, 64, 48, 512, "RGBA64_BE", hue90),
            lambda: g.submit_hsvfilter(ctx, d, 64, 48, 256, 12, hue90),
            lambda: g.submit_hsvfilter(ctx, d, 64, 48, 256, "RGBx", None),             # null settings
            lambda: g.submit_hsvfilter(ctx, d, 64, 48, 252, "RGBx", hue90),            # stride below the line bytes
            lambda: g.submit_hsvfilter(ctx, d, 64, 48, 191, "RGB", hue90),
            lambda: g.submit_hsvfilter(ctx, None, 64, 48, 256, "RGBx", hue90),         # null data with a non-empty frame
            lambda: g.submit_hsvfilter(ctx, d, -1, 48, 256, "RGBx", hue90),            # negative sizes
            lambda: g.submit_hsvfilter(ctx, d, 64, -1, 256, "RGBx", hue90),
            lambda: g.submit_hsvfilter(ctx, d, 64, 48, -256, "RGBx", hue90),
            lambda: g.wait_hsvfilter(0),                                               # unknown tickets
            lambda: g.wait_hsvfilter(12345),
        ]
        for call in bad:
            with pytest.raises(mi355fx.Mi355Error) as e:
                call()
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        s = mi355fx.HsvSettings(*hue90)
        t0 = C.c_uint64(0)
        assert g.L.mi355_group_submit_hsvfilter(g.h, None, d, 64, 48, 256, 0, C.byref(s), C.byref(t0)) == mi355fx.ERR_INVALID_ARG    # null ctx
        assert g.L.mi355_group_submit_hsvfilter(g.h, ctx.h, d, 64, 48, 256, 0, C.byref(s), None) == mi355fx.ERR_INVALID_ARG         # null ticket
        # the lone entry refuses the same frames with the same status
        for fmt, stride in (("RGBA64_LE", 512), ("RGBx", 252)):
            with pytest.raises(mi355fx.Mi355Error) as e:
                ctx.hsvfilter_frames_device(arena.dl + f.off, 1, 0, 64, 48, stride, fmt, hue90)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        t = f.submit(g)
        assert g.hsvfilter_stats() == (0, 0, 0, 0)                                     # a refused call queued and launched nothing
        # tickets of the other queues are refused here and stay collectable there
        t_pair = g.submit_compare(ctx, arena.dg + det_src.off, arena.dg + det_src.off, 256, 64, 48, "RGBA", 5)
        t_cd = g.submit_colordetect(ctx, arena.dg + det_src.off, 64 * 48 * 4, "RGBA", 10, 2)
        t_det = g.submit_hsvdetect(ctx, arena.dg + det_src.off, 256, "RGBx", arena.dg + det_dst.off, 256, "RGBA", 64, 48, (120.0, 40.0, 0.8, 0.5, 0.7, 0.6))
        t_chain = g.submit_chain(ctx, arena.dg + chain_src.off, arena.dg + chain_dst.off, 64, 48, 256, "RGBA", hue90)
        for other in (t_pair, t_cd, t_det, t_chain):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.wait_hsvfilter(other)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        # ... and the reverse
        for refuse in (g.wait, lambda tt: g.order_after(ctx, tt), g.wait_compare, g.wait_colordetect, g.wait_hsvdetect, g.wait_yolodec, g.wait_handdec):
            with pytest.raises(mi355fx.Mi355Error) as e:
                refuse(t)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.hsvfilter_stats() == (0, 0, 0, 0)
        assert g.wait_compare(t_pair)[0] == 0.0
        assert 1 <= len(g.wait_colordetect(t_cd)) <= 2
        g.wait_hsvdetect(t_det)
        g.wait(t_chain)
        assert g.hsvfilter_stats() == (0, 0, 0, 0)                                     # the other queues' launches are theirs
        g.wait_hsvfilter(t)
        assert g.hsvfilter_stats() == (1, 1, 1, 1)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_hsvfilter(t)                                                        # collected
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        # flush, then the waits in reverse order
        tk = [x.submit(g) for x in frames[1:3]]
        g.flush()
        assert g.hsvfilter_stats() == (3, 2, 2, 2)
        for tt in reversed(tk):
            g.wait_hsvfilter(tt)
        # wait_all covers the queue; the results stay collectable, once
        tk = [x.submit(g) for x in frames[3:]]
        g.wait_all()
        assert g.hsvfilter_stats() == (5, 3, 2, 4)                                     # a vector and a literal job
        for tt in tk:
            g.wait_hsvfilter(tt)
        with pytest.raises(mi355fx.Mi355Error):
            g.wait_hsvfilter(tk[0])
        # close() with frames pending launches them, waits and frees; a new group works
        runs = list(frames)
        frames[0].submit(g)
        frames[4].submit(g)
        g.close()
        runs += [frames[0], frames[4]]
        g = mi355fx.Group(0)
        g.wait_hsvfilter(frames[1].submit(g))
        runs.append(frames[1])
        assert g.hsvfilter_stats() == (1, 1, 1, 1)
        for run in runs:
            run.lone()
            run.expect(oracle)
        got_g, got_l = arena.read()
        theirs = np.zeros(arena.n, bool)
        for x in (det_dst, chain_src, chain_dst):
            theirs[x.off: x.off + x.nbytes] = True                                     # what the detector and the chain wrote, in the group's arena only: their own tests' business
        assert (got_g[~theirs] == got_l[~theirs]).all(), np.flatnonzero((got_g != got_l) & ~theirs)[:8]
        assert (got_g[~theirs] == arena.exp[~theirs]).all(), np.flatnonzero((got_g != arena.exp) & ~theirs)[:8]
    finally:
        g.close()
        arena.free()


def test_rendezvous_threads_fill_one_set(mi355lib, oracle):
    """Eight instances on eight threads, each with its own size, format and settings, submitting its frame and waiting at once (what
    transform_ip does): with a rendezvous of eight the frames of an interval share ONE launch set, unless somebody comes later than
    the linger."""
    import mi355fx
    n, rounds, linger = 8, 5, 0.2
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    arena = Arena(ctxs[0], n * (96 * 64 * 4 + 128) + 64)
    frames = [Frame(c, arena, 64 + 4 * s, 40 + s, FMTS[(s + 4) % 10], (FAST_SETTINGS + [GENERIC])[(3 * s) % 11], seed=90 + s, lead=(4 if s == 6 else 0))
              for s, c in enumerate(ctxs)]
    arena.upload()
    g = mi355fx.Group(0)
    g.set_hsvfilter_rendezvous(n, int(linger * 1e6))
    try:
        bar = threading.Barrier(n)
        errors = []
        submitted = [[0.0] * n for _ in range(rounds)]

        def element(s):
            try:
                for r in range(rounds):
                    bar.wait()
                    t = frames[s].submit(g)
                    submitted[r][s] = time.perf_counter()
                    g.wait_hsvfilter(t)
            except Exception as e:                 # noqa: BLE001 - told to the main thread
                errors.append(e)
                bar.abort()

        ts = [threading.Thread(target=element, args=(s,)) for s in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        st = g.hsvfilter_stats()
        # a member whose submit came more than half a linger behind its round's first may have missed that round's set
        late = [(r, s) for r in range(rounds) for s in range(n) if submitted[r][s] - min(submitted[r]) > linger / 2]
        assert st[0] == n * rounds
        assert rounds <= st[1] <= rounds + len(late), (st, late)
        assert late or st == (n * rounds, rounds, n, st[3])
        _finish(oracle, arena, [(f, f.c) for f in frames] * rounds)
    finally:
        g.close()
        arena.free()
        for c in ctxs:
            c.close()
