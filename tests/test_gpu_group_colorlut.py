"""GPU tests for the colorlut queue of the dispatcher (mi355_group_submit_colorlut / _wait_colorlut): the frames of INDEPENDENT
colorlut instances (one buffer per call and element: video/colorlut/src/colorlut/imp.rs:203-223), each with its own size, strides,
format and LUT, in shared launch sets - at most two launches over a job table: colorlut_jobs_kernel (four pixels per lane, the
per-axis cell index and weight of the 256 byte values tabled in LDS per block, the cells gathered from global memory) for RGBA
frames of the flat and rowpad classes, colorlut_rows_jobs_kernel (one pixel per lane, the body of colorlut_rows_kernel) for the rest.

The bar is `==` on the WHOLE arena against (a) Context.colorlut_frames_device with n_frames = 1 on a SECOND context holding the same
LUT, over a second arena prepared alike, and (b) the C oracle's colorlut over the host image. Every arena starts as a sentinel
pattern with the sources' pixels drawn into it and holds the bytes before an offset start, the row padding and 64 bytes behind each
plane, so an equal arena also proves that nothing outside the destination pixels was written and no source was touched.

One member of the issue's list cannot be as described: an RGBA 4 x 1 frame at an unpadded stride IS 16 bytes, a whole group, and the
flat class by the issue's own definition. It is kept at that size (and checked as flat), and a 3 x 1 frame - 12 bytes at an unpadded
stride - stands for "bytes that are no multiple of 16"."""
import ctypes as C
import json
import os
import threading
import time
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTOR, LITERAL = 1, 2
BPP = {"RGBA": 4, "RGBA64_LE": 8, "RGBA64_BE": 8}


class Lut:
    """One LUT in three places: the oracle's cube, a member context `g` (the one submitted with) and a second context `l` (the lone
    entry's)."""

    def __init__(self, cube, force_generic=False, lone_force_generic=False):
        import mi355fx
        self.cube = cube
        self.g, self.l = mi355fx.Context(0), mi355fx.Context(0)
        sc, of = cube.domain
        for c in (self.g, self.l):
            c.colorlut_load(cube.is3d, cube.size, cube.table, sc, of)
        if force_generic:
            self.g.set_flag(mi355fx.FLAG_FORCE_GENERIC, 1)
        if force_generic or lone_force_generic:
            self.l.set_flag(mi355fx.FLAG_FORCE_GENERIC, 1)

    def close(self):
        self.g.close()
        self.l.close()


def random_lut(oracle, is3d, size, seed, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), lo=-0.1, hi=1.1):
    rng = np.random.default_rng(seed)
    if is3d:
        t = np.ones((size ** 3, 4), np.float32)
        t[:, :3] = rng.uniform(lo, hi, (size ** 3, 3)).astype(np.float32)
    else:
        t = rng.uniform(lo, hi, 3 * size).astype(np.float32)
    return oracle.Cube.from_table(is3d, size, t, scale, offset)


class Arena:
    """Two device allocations prepared alike - the group works in one, the lone entry in the other - and the host image the oracle
    works in. Planes are carved from the same offsets of all three; `upload` sends the image once every source has its pixels."""

    def __init__(self, c, nbytes):
        self.c, self.n, self.top = c, nbytes, 0
        self.init = ((np.arange(nbytes, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
        self.exp = None
        self.dg, self.dl = c.alloc(nbytes), c.alloc(nbytes)
        assert self.dg % 16 == 0 and self.dl % 16 == 0

    def carve(self, nbytes, lead=0, tail=64):
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
    """One member's frame: a source and a destination plane of the arena. `src_at` / `dst_at` place a plane at a given offset (inside
    or on top of another frame's) instead of carving it; a carved source is drawn with seeded pixels (or `pixels`)."""

    def __init__(self, arena, lut, w, h, fmt="RGBA", seed=1, spad=0, dpad=0, lead=0, src_at=None, dst_at=None, pixels=None):
        self.arena, self.lut, self.w, self.h, self.fmt = arena, lut, w, h, fmt
        self.bpp = BPP[fmt]
        self.ss, self.ds = w * self.bpp + spad, w * self.bpp + dpad
        span = lambda stride: (h - 1) * stride + w * self.bpp if w > 0 and h > 0 else 0
        self.sbytes, self.dbytes = span(self.ss), span(self.ds)
        if src_at is None:
            self.soff = arena.carve(self.sbytes, lead=lead)
            rng = np.random.default_rng(seed)
            for r in range(h if w > 0 else 0):
                row = arena.init[self.soff + r * self.ss: self.soff + r * self.ss + w * self.bpp]
                row[:] = rng.integers(0, 256, row.size, dtype=np.uint8) if pixels is None else pixels[r * w * self.bpp: (r + 1) * w * self.bpp]
        else:
            self.soff = src_at
        self.doff = arena.carve(self.dbytes, lead=lead) if dst_at is None else dst_at

    def args(self, base):
        return (base + self.soff, self.ss, base + self.doff, self.ds, self.w, self.h, self.fmt)

    def plan_frame(self, force_generic=0):
        return self.args(self.arena.dg) + (force_generic,)

    def submit(self, g, c=None):
        return g.submit_colorlut(c or self.lut.g, *self.args(self.arena.dg))

    def lone(self):
        a = self.args(self.arena.dl)
        self.lut.l.colorlut_frames_device(a[0], 0, a[1], a[2], 0, a[3], 1, self.w, self.h, self.fmt)
        self.lut.l.synchronize()

    def expect(self, oracle):
        if not self.dbytes:
            return
        e = self.arena.exp
        src, dst = e[self.soff: self.soff + self.sbytes], e[self.doff: self.doff + self.dbytes]
        if self.fmt == "RGBA":
            oracle.colorlut_rgba8(self.lut.cube, src, self.ss, dst, self.ds, self.w, self.h)
        else:
            oracle.colorlut_rgba64(self.lut.cube, src, self.ss, dst, self.ds, self.w, self.h, le=self.fmt == "RGBA64_LE")

    def dst_pixels(self, image):
        rows = [image[self.doff + r * self.ds: self.doff + r * self.ds + self.w * self.bpp] for r in range(self.h)]
        return np.stack(rows).reshape(self.h, self.w * self.bpp)

    def src_pixels(self, image):
        rows = [image[self.soff + r * self.ss: self.soff + r * self.ss + self.w * self.bpp] for r in range(self.h)]
        return np.stack(rows).reshape(self.h, self.w * self.bpp)


def _finish(oracle, arena, frames):
    """Lone entry + oracle for every frame in the order given, then the whole-arena comparison."""
    for f in frames:
        f.lone()
        f.expect(oracle)
    got = arena.check()
    assert (got != arena.init).any()
    return got


def _plan(frames, force_generic=None):
    import mi355fx
    rc, n_sets, plan = mi355fx.selftest_colorlut_set_plan([f.plan_frame(int(bool(force_generic and force_generic[k]))) for k, f in enumerate(frames)])
    assert rc == 0
    return n_sets, plan


def test_unlike_members_one_set_two_launches(ctx, oracle, synth):
    import mi355fx
    dom = oracle.Cube.parse(synth.cube_text_3d(33, amp=0.06, domain=((-0.2, 0.05, 0.1), (1.3, 0.9, 1.0))))
    luts = {
        "3d33dom": Lut(dom),
        "3d17": Lut(oracle.Cube.parse(synth.cube_text_3d(17))),
        "3d2": Lut(random_lut(oracle, True, 2, 11)),
        "1d2": Lut(random_lut(oracle, False, 2, 12)),
        "1d1024": Lut(random_lut(oracle, False, 1024, 13, scale=(1.1, 0.9, 1.0), offset=(-0.05, 0.05, 0.0))),
    }
    arena = Arena(ctx, 64 * 1024)
    A = lambda *a, **k: Frame(arena, *a, **k)
    frames = [
        A(luts["3d33dom"], 64, 4, seed=1),                            # flat, 3D 33^3 with a non-trivial domain
        A(luts["3d17"], 5, 3, seed=2, spad=12, dpad=12),              # stride 32: rowpad, a tail of 1
        A(luts["3d17"], 6, 2, seed=3, spad=8, dpad=8),                # stride 32: a tail of 2
        A(luts["3d33dom"], 7, 2, seed=4, lead=4),                     # base + 4: literal
        A(luts["3d17"], 4, 1, seed=5),                                # 16 bytes at an unpadded stride: one whole group (module docstring)
        A(luts["3d17"], 3, 1, seed=6),                                # 12 bytes at an unpadded stride: literal
        A(luts["3d33dom"], 3, 2, "RGBA64_LE", seed=7),
        A(luts["3d33dom"], 3, 2, "RGBA64_BE", seed=8, spad=16, dpad=8),
        A(luts["1d2"], 16, 3, seed=9),
        A(luts["1d2"], 5, 2, "RGBA64_LE", seed=10),
        A(luts["1d1024"], 9, 5, seed=11, spad=12, dpad=28),           # rowpad, unlike strides (48 and 64), a tail of 1
        A(luts["1d1024"], 5, 2, "RGBA64_BE", seed=12),
        A(luts["3d2"], 12, 3, seed=13),
        A(luts["3d2"], 7, 3, seed=14, spad=4, dpad=4),                # stride 32: a tail of 3
        A(luts["3d17"], 33, 9, seed=15, lead=8),                      # literal, more than one block
    ]
    arena.upload()
    g = mi355fx.Group(0)
    g.set_colorlut_rendezvous(len(frames), 5_000_000)
    try:
        n_sets, plan = _plan(frames)
        assert n_sets == 1
        assert [p["launch"] for p in plan] == [1, 1, 1, 2, 1, 2, 2, 2, 1, 2, 1, 2, 1, 1, 2]
        assert [p["geometry"] for p in plan] == [1, 2, 2, 0, 1, 0, 0, 0, 1, 0, 2, 0, 1, 2, 0]
        assert plan[14]["blocks"] == 2
        tk = [f.submit(g) for f in frames[:-1]]
        assert g.colorlut_stats() == (0, 0, 0, 0)                     # nothing goes out before the rendezvous is complete
        tk.append(frames[-1].submit(g))
        assert g.colorlut_stats() == (15, 1, 15, 2)                   # one set, two launches
        for t in reversed(tk):
            g.wait_colorlut(t)
        assert g.colorlut_stats() == (15, 1, 15, 2)
        _finish(oracle, arena, frames)
    finally:
        g.close()
        arena.free()
        for lut in luts.values():
            lut.close()


def test_all_colours_through_the_vector_kernel(ctx, oracle, synth):
    """All 2^24 colours, three LUTs, one set - the squeezed plan: three jobs want 3 x 8192 blocks of the 256 x 16 there are, so every
    block runs its stride loop several times. Pins, colour by colour, that the tabled index and weight plus sample_3d_at / sample_1d_at
    are the lone routes' arithmetic."""
    import mi355fx
    with open(os.path.join(ROOT, "tests", "golden", "pixel_crc.json")) as fh:
        golden = json.load(fh)["crc32"]
    cases = [("lut33", synth.cube_text_3d(33)),
             ("lut17_domain", synth.cube_text_3d(17, amp=0.07, domain=((-0.25, 0.0, 0.1), (1.5, 1.0, 0.9)))),   # clamps on both sides (blue: below 0.1, above 0.9)
             ("lut1d64", synth.cube_text_1d(64))]
    allc = synth.allcolors().reshape(-1)
    n = allc.nbytes
    src = ctx.alloc(n)
    ctx.h2d(src, allc)
    luts = [Lut(oracle.Cube.parse(text)) for _, text in cases]
    dsts = [(ctx.alloc(n), ctx.alloc(n)) for _ in cases]
    g = mi355fx.Group(0)
    g.set_colorlut_rendezvous(len(cases), 5_000_000)
    try:
        rc, n_sets, plan = mi355fx.selftest_colorlut_set_plan([(src, 16384, dg, 16384, 4096, 4096, "RGBA") for dg, _ in dsts])
        assert rc == 0 and n_sets == 1 and all(p["launch"] == VECTOR and p["geometry"] == 1 for p in plan)
        assert all(p["blocks"] < -(-p["units"] // 512) for p in plan)                        # squeezed
        tk = [g.submit_colorlut(lut.g, src, 16384, dg, 16384, 4096, 4096, "RGBA") for lut, (dg, _) in zip(luts, dsts)]
        assert g.colorlut_stats() == (3, 1, 3, 1)                                            # three members that share a source: one set, one launch
        for t in tk:
            g.wait_colorlut(t)
        for (tag, _), lut, (dg, dl) in zip(cases, luts, dsts):
            lut.l.colorlut_frames_device(src, 0, 16384, dl, 0, 16384, 1, 4096, 4096, "RGBA")
            lut.l.synchronize()
            got_g, got_l, exp = np.empty_like(allc), np.empty_like(allc), np.zeros_like(allc)
            ctx.d2h(got_g, dg)
            ctx.d2h(got_l, dl)
            oracle.colorlut_rgba8(lut.cube, allc, 16384, exp, 16384, 4096, 4096, nthreads=16)
            assert (got_g == got_l).all(), (tag, np.flatnonzero(got_g != got_l)[:8])
            assert (got_g == exp).all(), (tag, np.flatnonzero(got_g != exp)[:8])
            assert zlib.crc32(got_g.tobytes()) == golden["colorlut_allcolors_" + tag], tag
    finally:
        g.close()
        ctx.free(src)
        for dg, dl in dsts:
            ctx.free(dg)
            ctx.free(dl)
        for lut in luts:
            lut.close()


def _ramps():
    """RGBA 256 x 4: every byte value on every axis (rising, falling, a stride of 7 and constant rows), the alpha byte = the column."""
    v = np.arange(256, dtype=np.uint8)
    px = np.zeros((4, 256, 4), np.uint8)
    px[0, :, 0], px[0, :, 1], px[0, :, 2] = v, v, v
    px[1, :, 0], px[1, :, 1], px[1, :, 2] = v, 255 - v, v * 7
    px[2, :, 0], px[2, :, 1], px[2, :, 2] = 255, v, 0
    px[3, :, 0], px[3, :, 1], px[3, :, 2] = v * 7, 255, 255 - v
    px[:, :, 3] = v
    return px.reshape(-1)


def _ramps64(le):
    """RGBA64 256 x 256: the alpha word takes every value; the colour words sweep the axes, the ends 0 and 65535 included."""
    i = np.arange(65536, dtype=np.uint32)
    px = np.zeros((65536, 4), np.uint16)
    px[:, 0], px[:, 1], px[:, 2], px[:, 3] = i, 65535 - i, (i * 257) & 0xffff, i
    px[:256, :3] = np.arange(256, dtype=np.uint16)[:, None] * 257      # 0, 257, ... 65535 on all three axes at once
    return px.astype("<u2" if le else ">u2").view(np.uint8).reshape(-1)


def test_edges_of_the_arithmetic(ctx, oracle):
    import mi355fx
    ident3 = np.ones((8, 4), np.float32)
    for i in range(8):
        ident3[i, :3] = (i & 1, i >> 1 & 1, i >> 2)
    wild = np.ones((27, 4), np.float32)
    wild[:, :3] = np.random.default_rng(5).uniform(0, 1, (27, 3)).astype(np.float32)
    wild[1, 0], wild[3, 1], wild[5, 2], wild[7, 0] = np.nan, np.inf, -np.inf, 1e38
    wild[13, :3] = (1e38, -1e38, np.nan)
    wild[20, 1], wild[26, 2], wild[0, 2] = -1e38, np.inf, np.nan
    wild1 = np.random.default_rng(6).uniform(0, 1, 3 * 5).astype(np.float32)
    wild1[[1, 6, 12, 4, 9]] = (np.nan, np.inf, -np.inf, 1e38, -1e38)
    luts = [
        Lut(oracle.Cube.from_table(True, 2, ident3)),                                                     # scale 1: input 255 is x == size - 1 exactly
        Lut(random_lut(oracle, True, 5, 21)),                                                             # ... and in a LUT with inner cells
        Lut(random_lut(oracle, True, 4, 22, scale=(0.0, 1.0, -0.0))),                                     # zero scales
        Lut(random_lut(oracle, True, 4, 23, scale=(-1.0, -0.5, 1.0), offset=(1.0, 0.75, 0.0))),           # negative scales
        Lut(random_lut(oracle, True, 4, 24, scale=(1.0, 2.0, 0.5), offset=(2.0, -1.0, -0.5))),            # offsets beyond [0, 1]: clamped above, below, below
        Lut(random_lut(oracle, False, 7, 25, scale=(-2.0, 0.0, 3.0), offset=(1.5, 7.0, -1.0))),           # the same on a 1D LUT
        Lut(random_lut(oracle, False, 2, 26)),
        Lut(oracle.Cube.from_table(True, 3, wild, (1.0, 1.1, 0.9), (0.0, -0.05, 0.1)), lone_force_generic=True),   # NaN, +-inf and 1e38 in the cells
        Lut(oracle.Cube.from_table(False, 5, wild1), lone_force_generic=True),
    ]
    arena = Arena(ctx, len(luts) * (4096 + 2 * 524288 + 4 * 1024) * 2 + 4096)
    frames = []
    for k, lut in enumerate(luts):
        frames.append(Frame(arena, lut, 256, 4, pixels=_ramps()))                                         # vector
        frames.append(Frame(arena, lut, 256, 256, "RGBA64_LE" if k % 2 else "RGBA64_BE", pixels=_ramps64(k % 2 == 1)))   # literal
    arena.upload()
    g = mi355fx.Group(0)
    g.set_colorlut_rendezvous(len(frames), 5_000_000)
    try:
        n_sets, plan = _plan(frames)
        assert n_sets == 1 and [p["launch"] for p in plan] == [VECTOR, LITERAL] * len(luts)
        tk = [f.submit(g) for f in frames]
        assert g.colorlut_stats() == (len(frames), 1, len(frames), 2)
        for t in tk:
            g.wait_colorlut(t)
        got = _finish(oracle, arena, frames)
        # input 255 at scale 1 through the identity LUT: the clamped corner with weight 0 gives 255 back, and every other value itself
        out = frames[0].dst_pixels(got).reshape(4, 256, 4)
        assert (out == _ramps().reshape(4, 256, 4)).all()
        # alpha byte and alpha word, every value, unchanged
        for f in frames:
            a_in, a_out = f.src_pixels(arena.init), f.dst_pixels(got)
            if f.fmt == "RGBA":
                assert (a_out[:, 3::4] == a_in[:, 3::4]).all() and len(np.unique(a_in[:, 3::4])) == 256
            else:
                w_in, w_out = a_in.reshape(-1, 8)[:, 6:], a_out.reshape(-1, 8)[:, 6:]
                assert (w_out == w_in).all() and len(np.unique(w_in.copy().view(np.uint16))) == 65536
    finally:
        g.close()
        arena.free()
        for lut in luts:
            lut.close()


def test_order_across_frames(ctx, oracle, synth):
    import mi355fx
    la, lb = Lut(oracle.Cube.parse(synth.cube_text_3d(17))), Lut(random_lut(oracle, True, 9, 31))
    arena = Arena(ctx, 64 * 1024)
    # B's source is A's destination: two LUTs chained through the queue
    a1 = Frame(arena, la, 32, 8, seed=41)
    b1 = Frame(arena, lb, 32, 8, src_at=a1.doff)
    # B's destination meets A's destination: the later one wins (B writes a sub-rectangle of what A writes)
    a2 = Frame(arena, la, 32, 8, seed=42)
    b2 = Frame(arena, lb, 8, 4, seed=43, dpad=(32 - 8) * 4, dst_at=a2.doff + 2 * a2.ds + 5 * 4)
    # B's destination meets A's source: A reads the old bytes
    a3 = Frame(arena, la, 32, 8, seed=44)
    b3 = Frame(arena, lb, 32, 8, seed=45, dst_at=a3.soff)
    arena.upload()
    g = mi355fx.Group(0)
    try:
        for k, (a, b) in enumerate(((a1, b1), (a2, b2), (a3, b3))):
            assert _plan([a, b])[0] == 2
            ta = a.submit(g)
            assert g.colorlut_stats()[:2] == (2 * k, 2 * k)
            tb = b.submit(g)                                          # what was pending goes out first
            assert g.colorlut_stats()[:2] == (2 * k + 1, 2 * k + 1)
            g.wait_colorlut(tb)
            g.wait_colorlut(ta)
            assert g.colorlut_stats() == (2 * k + 2, 2 * k + 2, 1, 2 * k + 2)                # two sets per pair
        got = _finish(oracle, arena, [a1, b1, a2, b2, a3, b3])
        # the order is visible in each pair: the other order gives other bytes
        other = arena.init.copy()
        arena.exp = other
        for f in (b1, a1, b2, a2, b3, a3):
            f.expect(oracle)
        assert (b1.dst_pixels(other) != b1.dst_pixels(got)).any()
        assert (a2.dst_pixels(other) != a2.dst_pixels(got)).any()
        assert (a3.dst_pixels(other) != a3.dst_pixels(got)).any()
    finally:
        g.close()
        arena.free()
        la.close()
        lb.close()


def test_set_mechanics(ctx, oracle, synth):
    import mi355fx
    lut = Lut(oracle.Cube.parse(synth.cube_text_3d(9)))
    forced = Lut(oracle.Cube.parse(synth.cube_text_3d(9)), force_generic=True)
    one_d = Lut(random_lut(oracle, False, 16, 51))
    arena = Arena(ctx, 128 * 1024)
    many = [Frame(arena, (lut, one_d)[k % 2], 4 + k % 5, 1 + k % 3, ("RGBA", "RGBA", "RGBA64_LE")[k % 3], seed=60 + k) for k in range(33)]
    gen = [Frame(arena, forced, 64, 4, seed=95), Frame(arena, forced, 5, 3, seed=96, spad=12, dpad=12), Frame(arena, forced, 6, 3, "RGBA64_BE", seed=97)]
    same = [Frame(arena, lut, 64, 4, seed=95), Frame(arena, lut, 5, 3, seed=96, spad=12, dpad=12)]    # the forced members' RGBA frames through the vector launch
    arena.upload()
    g = mi355fx.Group(0)
    try:
        # 33 frames make two sets
        tk = [f.submit(g) for f in many]
        assert g.colorlut_stats()[:3] == (32, 1, 32)                  # the 32nd submit filled a set
        for t in tk:
            g.wait_colorlut(t)
        assert g.colorlut_stats()[:3] == (33, 2, 32)
        # FORCE_GENERIC members go literal; two members share one context - and therefore one LUT - in one set
        n_sets, plan = _plan(gen + same, force_generic=[1, 1, 1, 0, 0])
        assert n_sets == 1 and [p["launch"] for p in plan] == [LITERAL] * 3 + [VECTOR] * 2
        before = g.colorlut_stats()
        tk = [f.submit(g) for f in gen + same]
        for t in reversed(tk):
            g.wait_colorlut(t)
        after = g.colorlut_stats()
        assert (after[0] - before[0], after[1] - before[1], after[3] - before[3]) == (5, 1, 2)
        got = _finish(oracle, arena, many + gen + same)
        for a, b in zip(gen[:2], same):
            assert (a.dst_pixels(got) == b.dst_pixels(got)).all()    # the same bytes through either launch
    finally:
        g.close()
        arena.free()
        for x in (lut, forced, one_d):
            x.close()


def test_a_frame_is_converted_after_what_its_stream_held(ctx, oracle, synth):
    """The member's source is written by lone launches queued asynchronously on the member's own stream - its own LUT over a first
    picture, three times round - and the group submit follows at once, no host wait between: the set runs behind them."""
    import mi355fx
    w, h = 1920, 1080
    lut = Lut(oracle.Cube.parse(synth.cube_text_3d(33)))
    arena = Arena(ctx, 3 * (w * h * 4 + 128) + 64)
    first = Frame(arena, lut, w, h, pixels=synth.smooth_frame(w, h).reshape(-1))
    back = Frame(arena, lut, w, h, src_at=first.doff, dst_at=first.soff)
    f = Frame(arena, lut, w, h, src_at=first.doff)
    arena.upload()
    g = mi355fx.Group(0)
    try:
        a, b = first.args(arena.dg), back.args(arena.dg)
        for x in (a, b, a, b, a):
            lut.g.colorlut_frames_device(x[0], 0, x[1], x[2], 0, x[3], 1, w, h, "RGBA")
        g.wait_colorlut(f.submit(g))
        # the lone arena and the oracle: the same five calls (on the second context), then the frame
        for x in (first, back, first, back, first):
            x.lone()
            x.expect(oracle)
        _finish(oracle, arena, [f])
    finally:
        g.close()
        arena.free()
        lut.close()


def test_protocol(ctx, oracle, synth):
    import mi355fx
    lut = Lut(oracle.Cube.parse(synth.cube_text_3d(17)))
    bare = mi355fx.Context(0)                                                      # no LUT
    ctx.colorlut_load(lut.cube.is3d, lut.cube.size, lut.cube.table, *lut.cube.domain)   # (the chain of the foreign tickets needs one)
    arena = Arena(ctx, 256 * 1024)
    frames = [Frame(arena, lut, 64, 48, seed=100 + k) for k in range(4)] + [Frame(arena, lut, 33, 21, "RGBA64_LE", seed=105)]
    valid = [Frame(arena, lut, 8, 2, seed=110 + k) for k in range(16)]
    other_src, other_dst, chain = Frame(arena, lut, 64, 48, seed=130), Frame(arena, lut, 64, 48, seed=131), Frame(arena, lut, 64, 48, seed=132)
    arena.upload()
    g = mi355fx.Group(0)
    try:
        f = frames[0]
        s, d = arena.dg + f.soff, arena.dg + f.doff
        sub = lambda *a: g.submit_colorlut(lut.g, *a)
        bad = [
            (lambda: sub(s, 256, d, 256, 64, 48, "RGBx"), mi355fx.ERR_INVALID_ARG),            # not one of the three formats
            (lambda: sub(s, 256, d, 256, 64, 48, "BGRA"), mi355fx.ERR_INVALID_ARG),
            (lambda: sub(s, 192, d, 192, 64, 48, "RGB"), mi355fx.ERR_INVALID_ARG),
            (lambda: sub(s, 256, d, 256, 64, 48, 12), mi355fx.ERR_INVALID_ARG),
            (lambda: g.submit_colorlut(bare, s, 256, d, 256, 64, 48, "RGBA"), mi355fx.ERR_NOT_CONFIGURED),   # no LUT
            (lambda: g.submit_colorlut(bare, s, 256, d, 256, 64, 48, "RGBx"), mi355fx.ERR_INVALID_ARG),      # ... the format is looked at first
            (lambda: g.submit_colorlut(bare, s, 256, d, 256, -1, 48, "RGBA"), mi355fx.ERR_NOT_CONFIGURED),   # ... the sizes after it
            (lambda: sub(s, 256, d, 256, -1, 48, "RGBA"), mi355fx.ERR_INVALID_ARG),            # negative sizes
            (lambda: sub(s, 256, d, 256, 64, -1, "RGBA"), mi355fx.ERR_INVALID_ARG),
            (lambda: sub(None, 256, d, 256, 64, 48, "RGBA"), mi355fx.ERR_INVALID_ARG),         # null data with a pixel
            (lambda: sub(s, 256, None, 256, 64, 48, "RGBA"), mi355fx.ERR_INVALID_ARG),
            (lambda: sub(s, 252, d, 256, 64, 48, "RGBA"), mi355fx.ERR_INVALID_ARG),            # strides below the row bytes
            (lambda: sub(s, 256, d, 252, 64, 48, "RGBA"), mi355fx.ERR_INVALID_ARG),
            (lambda: sub(s, 511, d, 512, 64, 48, "RGBA64_LE"), mi355fx.ERR_INVALID_ARG),
            (lambda: sub(s, 256, s, 256, 64, 48, "RGBA"), mi355fx.ERR_INVALID_ARG),            # the queue's own: source and destination meet
            (lambda: sub(s, 256, s + f.sbytes - 1, 256, 64, 48, "RGBA"), mi355fx.ERR_INVALID_ARG),
        ]
        assert len(bad) == len(valid)
        tk = []
        for (call, status), ok in zip(bad, valid):                                 # every refusal, each followed by a valid frame
            with pytest.raises(mi355fx.Mi355Error) as e:
                call()
            assert e.value.status == status
            tk.append(ok.submit(g))
        t0 = C.c_uint64(0)
        assert g.L.mi355_group_submit_colorlut(g.h, None, s, 256, d, 256, 64, 48, 4, C.byref(t0)) == mi355fx.ERR_INVALID_ARG       # null ctx
        assert g.L.mi355_group_submit_colorlut(g.h, lut.g.h, s, 256, d, 256, 64, 48, 4, None) == mi355fx.ERR_INVALID_ARG           # null ticket
        # the lone entry refuses the same frames with the same status
        for c, args, status in ((lut.l, (s, 0, 256, d, 0, 256, 1, 64, 48, "RGBx"), mi355fx.ERR_INVALID_ARG), (bare, (s, 0, 256, d, 0, 256, 1, 64, 48, "RGBA"), mi355fx.ERR_NOT_CONFIGURED),
                                (bare, (s, 0, 256, d, 0, 256, 1, -1, 48, "RGBA"), mi355fx.ERR_NOT_CONFIGURED), (lut.l, (s, 0, 252, d, 0, 256, 1, 64, 48, "RGBA"), mi355fx.ERR_INVALID_ARG)):
            with pytest.raises(mi355fx.Mi355Error) as e:
                c.colorlut_frames_device(*args)
            assert e.value.status == status
        assert g.colorlut_stats() == (0, 0, 0, 0)                                  # the refused calls queued nothing, the valid ones wait
        for t in tk:
            g.wait_colorlut(t)
        assert g.colorlut_stats() == (16, 1, 16, 1)
        # empty frames: a ticket, no launch, null pointers are fine
        tk = [g.submit_colorlut(lut.g, s, 256, d, 256, 0, 48, "RGBA"), g.submit_colorlut(lut.g, None, 0, None, 0, 0, 0, "RGBA64_BE"),
              g.submit_colorlut(lut.g, s, 0, s, 0, 16, 0, "RGBA")]
        for t in tk:
            g.wait_colorlut(t)
        assert g.colorlut_stats() == (19, 2, 16, 1)
        # unknown tickets, a double wait
        for t in (0, 12345, tk[0]):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.wait_colorlut(t)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        # tickets of the other queues are refused here and stay collectable there
        t = f.submit(g)
        hue90 = (90.0, 1.25, -0.05, 0.8, 0.1)
        o_s, o_d = arena.dg + other_src.soff, arena.dg + other_dst.doff
        t_pair = g.submit_compare(ctx, o_s, o_s, 256, 64, 48, "RGBA", 5)
        t_cd = g.submit_colordetect(ctx, o_s, 64 * 48 * 4, "RGBA", 10, 2)
        t_det = g.submit_hsvdetect(ctx, o_s, 256, "RGBx", o_d, 256, "RGBA", 64, 48, (120.0, 40.0, 0.8, 0.5, 0.7, 0.6))
        t_hf = g.submit_hsvfilter(ctx, arena.dg + other_dst.soff, 64, 48, 256, "RGBA", hue90)
        t_chain = g.submit_chain(ctx, arena.dg + chain.soff, arena.dg + chain.doff, 64, 48, 256, "RGBA", hue90)
        for other in (t_pair, t_cd, t_det, t_hf, t_chain):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.wait_colorlut(other)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        # ... and the reverse
        for refuse in (g.wait, lambda tt: g.order_after(ctx, tt), g.wait_compare, g.wait_colordetect, g.wait_hsvdetect, g.wait_hsvfilter, g.wait_yolodec, g.wait_handdec):
            with pytest.raises(mi355fx.Mi355Error) as e:
                refuse(t)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.colorlut_stats() == (19, 2, 16, 1)
        assert g.wait_compare(t_pair)[0] == 0.0
        assert 1 <= len(g.wait_colordetect(t_cd)) <= 2
        g.wait_hsvdetect(t_det)
        g.wait_hsvfilter(t_hf)
        g.wait(t_chain)
        assert g.colorlut_stats() == (19, 2, 16, 1)                                # the other queues' launches are theirs
        g.wait_colorlut(t)
        assert g.colorlut_stats() == (20, 3, 16, 2)
        # flush, then the waits in reverse order
        tk = [x.submit(g) for x in frames[1:3]]
        g.flush()
        assert g.colorlut_stats() == (22, 4, 16, 3)
        for tt in reversed(tk):
            g.wait_colorlut(tt)
        # wait_all covers the queue; the results stay collectable, once
        tk = [x.submit(g) for x in frames[3:]]
        g.wait_all()
        assert g.colorlut_stats() == (24, 5, 16, 5)                                # a vector and a literal job
        for tt in tk:
            g.wait_colorlut(tt)
        with pytest.raises(mi355fx.Mi355Error):
            g.wait_colorlut(tk[0])
        # close() with frames pending launches them, waits and frees; a new group works
        runs = valid + frames
        frames[0].submit(g)
        frames[4].submit(g)
        g.close()
        g = mi355fx.Group(0)
        g.wait_colorlut(frames[1].submit(g))
        assert g.colorlut_stats() == (1, 1, 1, 1)
        for run in runs:
            run.lone()
            run.expect(oracle)
        got_g, got_l = arena.read()
        theirs = np.zeros(arena.n, bool)
        for off, nbytes in ((other_dst.doff, other_dst.dbytes), (other_dst.soff, other_dst.sbytes), (chain.soff, chain.sbytes), (chain.doff, chain.dbytes)):
            theirs[off: off + nbytes] = True                                       # what the detector, the filter and the chain wrote, in the group's arena only: their own tests' business
        assert (got_g[~theirs] == got_l[~theirs]).all(), np.flatnonzero((got_g != got_l) & ~theirs)[:8]
        assert (got_g[~theirs] == arena.exp[~theirs]).all(), np.flatnonzero((got_g != arena.exp) & ~theirs)[:8]
    finally:
        g.close()
        arena.free()
        lut.close()
        bare.close()


def test_rendezvous_threads_fill_one_set(mi355lib, oracle, synth):
    """Eight instances on eight threads, each with its own size, format and LUT, submitting its frame and waiting at once (what the
    element's generate_output does): with a rendezvous of eight the frames of an interval share ONE launch set, unless somebody
    comes later than the linger."""
    import mi355fx
    n, rounds, linger = 8, 5, 0.2
    luts = [Lut(random_lut(oracle, s % 3 != 2, (33, 17, 1024, 2, 9, 64, 5, 12)[s], 140 + s)) for s in range(n)]
    arena = Arena(luts[0].g, n * 2 * (96 * 64 * 8 + 128) + 64)
    frames = [Frame(arena, luts[s], 64 + 4 * s, 40 + s, ("RGBA", "RGBA", "RGBA64_LE", "RGBA", "RGBA64_BE")[s % 5], seed=150 + s, lead=(4 if s == 6 else 0),
                    spad=(16 if s == 3 else 0), dpad=(32 if s == 3 else 0)) for s in range(n)]
    arena.upload()
    g = mi355fx.Group(0)
    g.set_colorlut_rendezvous(n, int(linger * 1e6))
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
                    g.wait_colorlut(t)
            except Exception as e:                 # noqa: BLE001 - told to the main thread
                errors.append(e)
                bar.abort()

        ts = [threading.Thread(target=element, args=(s,)) for s in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        st = g.colorlut_stats()
        # a member whose submit came more than half a linger behind its round's first may have missed that round's set
        late = [(r, s) for r in range(rounds) for s in range(n) if submitted[r][s] - min(submitted[r]) > linger / 2]
        assert st[0] == n * rounds
        assert rounds <= st[1] <= rounds + len(late), (st, late)
        assert late or st == (n * rounds, rounds, n, 2 * rounds)
        _finish(oracle, arena, frames)
    finally:
        g.close()
        arena.free()
        for lut in luts:
            lut.close()
