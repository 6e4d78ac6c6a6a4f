"""GPU tests for the hsvdetector queue of the dispatcher (mi355_group_submit_hsvdetect / _wait_hsvdetect): the frames of
INDEPENDENT hsvdetector instances (one buffer per call and element, video/hsv/src/hsvdetector/imp.rs:423-707) in shared launch
sets - at most two launches over a job table: hsvdetect_jobs_kernel (four pixels per lane) for the frames the lone entry gives
to its flat or rgb24 kernel, hsvdetect_rows_jobs_kernel (literal, one pixel per lane) for the rest. Members differ in size,
strides, alignment, input and output format and settings.

The bar is `==` on the WHOLE destination arena against (a) Context.hsvdetect_frames_device on the same device bytes, written
into a second arena prepared the same way, and (b) oracle.hsvdetect on the host copy. Every arena starts as a sentinel pattern
and holds the bytes before an offset start, the row padding and at least 64 bytes past each frame, so an equal arena also proves
that nothing outside the pixels was written. Each test asserts that both alpha values occur in its set."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ST = (120.0, 40.0, 0.8, 0.5, 0.7, 0.6)      # hue_ref, hue_var, saturation_ref, saturation_var, value_ref, value_var
IN4 = ("RGBx", "xRGB", "BGRx", "xBGR")
IN_FMTS = IN4 + ("RGB", "BGR")
OUT_FMTS = ("RGBA", "ARGB", "BGRA", "ABGR")
OUT_LAYOUT = {"RGBA": (False, False), "ARGB": (True, False), "BGRA": (False, True), "ABGR": (True, True)}   # alpha first, bgr


def _st(hue_ref, **kw):
    s = list(ST)
    s[0] = hue_ref
    for k, v in kw.items():
        s[{"hue_var": 1, "sat_ref": 2, "sat_var": 3, "val_ref": 4, "val_var": 5}[k]] = v
    return tuple(s)


class Arena:
    """Two device allocations prepared alike - the group writes into one, the lone entry into the other - and the host image
    the oracle writes into. Frames are carved from the same offsets of all three."""

    def __init__(self, c, nbytes):
        self.c, self.n, self.top = c, nbytes, 0
        self.sentinel = ((np.arange(nbytes, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
        self.exp = self.sentinel.copy()
        self.dg, self.dl = c.alloc(nbytes), c.alloc(nbytes)
        assert self.dg % 16 == 0 and self.dl % 16 == 0
        c.h2d(self.dg, self.sentinel)
        c.h2d(self.dl, self.sentinel)

    def carve(self, nbytes, lead=0, tail=64):
        """`nbytes` at a 16-byte aligned offset + lead, `tail` sentinel bytes behind it."""
        off = (self.top + 15) // 16 * 16 + lead
        self.top = off + nbytes + tail
        assert self.top <= self.n, "arena too small"
        return off

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
    """One member's frame: its source on the device (its own allocation, `src_off` bytes in) and its destination in the arena."""

    def __init__(self, c, arena, w, h, in_fmt, out_fmt, st, seed=1, src_pad=0, dst_pad=0, src_off=0, dst_off=0, tail=64, host=None, share=None):
        from mi355fx import FMT_LAYOUT
        self.c, self.arena, self.w, self.h, self.in_fmt, self.out_fmt, self.st = c, arena, w, h, in_fmt, out_fmt, st
        self.ps, self.first, self.bgr = FMT_LAYOUT[in_fmt]
        self.ss, self.ds = w * self.ps + src_pad, w * 4 + dst_pad
        if share is not None:                      # the same device bytes as another frame
            self.host, self.salloc, self.dsrc = share.host, None, share.dsrc
        else:
            n = h * self.ss
            self.host = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8) if host is None else np.ascontiguousarray(host, np.uint8).reshape(-1)
            assert self.host.nbytes == n
            self.salloc = c.alloc(src_off + n + 16)
            self.dsrc = self.salloc + src_off
            if n:
                c.h2d(self.dsrc, self.host)
        self.off = arena.carve(h * self.ds, lead=dst_off, tail=tail)

    def submit(self, g, c=None):
        return g.submit_hsvdetect(c or self.c, self.dsrc, self.ss, self.in_fmt, self.arena.dg + self.off, self.ds, self.out_fmt, self.w, self.h, self.st)

    def lone(self, c=None):
        (c or self.c).hsvdetect_frames_device(self.dsrc, 0, self.ss, self.in_fmt, self.arena.dl + self.off, 0, self.ds, self.out_fmt, 1, self.w, self.h, self.st)
        (c or self.c).synchronize()

    def expect(self, oracle):
        """The oracle's frame into the arena's host image; returns the alpha bytes."""
        if self.w == 0 or self.h == 0:
            return np.zeros(0, np.uint8)
        af, obgr = OUT_LAYOUT[self.out_fmt]
        dst = self.arena.exp[self.off: self.off + self.h * self.ds]
        oracle.hsvdetect(self.host, self.ss, self.ps, self.first, bool(self.bgr), dst, self.ds, af, obgr, self.w, self.st)
        return dst.reshape(self.h, self.ds)[:, (0 if af else 3): self.w * 4: 4].reshape(-1)

    def free(self):
        if self.salloc:
            self.c.free(self.salloc)
            self.salloc = None


def _finish(oracle, arena, frames, members=None):
    """Lone entry + oracle for every frame, the whole-arena comparison, and both alpha values somewhere in the set."""
    alphas = []
    for k, f in enumerate(frames):
        f.lone(members[k] if members else None)
        alphas.append(f.expect(oracle))
    got = arena.check()
    a = np.concatenate(alphas)
    assert set(np.unique(a).tolist()) == {0, 255}, np.unique(a)
    return got


def _free(g, arena, frames):
    if g is not None:
        g.close()
    for f in frames:
        f.free()
    arena.free()


def test_unlike_members_one_set_one_launch(ctx, oracle):
    """Ten vector-class members: every input format, every output format, both offset classes and their edges, one group to
    eight blocks per job. Destinations back to back in one allocation: an overrun lands in a neighbour."""
    import mi355fx
    arena = Arena(ctx, 192 * 1024)
    mk = lambda w, h, i, o, hue, seed: Frame(ctx, arena, w, h, i, o, _st(hue), seed=seed, tail=0)
    frames = [
        mk(16, 3, "RGBx", "RGBA", 120.0, 1),
        mk(4, 1, "xRGB", "ARGB", 240.0, 2),               # one 16-byte group
        mk(64, 48, "BGRx", "BGRA", -180.0, 3),            # off = 360
        mk(16, 3, "xBGR", "ABGR", 180.00002, 4),          # off just below 0
        mk(64, 48, "RGB", "ARGB", 540.0, 5),              # off = -360
        mk(16, 3, "BGR", "RGBA", 240.0, 6),
        mk(256, 64, "RGBx", "ABGR", 240.0, 7),            # 4096 groups: eight blocks
        mk(4, 1, "BGR", "BGRA", 120.0, 8),
        mk(64, 48, "xBGR", "RGBA", 120.0, 9),
        mk(256, 64, "RGB", "BGRA", 120.0, 10),            # eight blocks of 12-byte loads
    ]
    g = mi355fx.Group(0)
    try:
        assert all(f.off % 16 == 0 and f.dsrc % 16 == 0 for f in frames)
        assert all(a.off + a.h * a.ds == b.off for a, b in zip(frames, frames[1:]))      # back to back
        tk = [f.submit(g) for f in frames]
        assert g.hsvdetect_stats() == (0, 0, 0, 0)                                        # nothing goes out before a wait or a full set
        for t in reversed(tk):
            g.wait_hsvdetect(t)
        n = len(frames)
        assert g.hsvdetect_stats() == (n, 1, n, 1)
        _finish(oracle, arena, frames)
    finally:
        _free(g, arena, frames)


def test_the_literal_class_each_cause_alone_and_both_classes_in_one_set(ctx, oracle):
    import mi355fx
    arena = Arena(ctx, 64 * 1024)
    generic = mi355fx.Context(0)
    generic.set_flag(mi355fx.FLAG_FORCE_GENERIC, 1)
    literal = [
        Frame(ctx, arena, 16, 3, "RGBx", "RGBA", ST, seed=1, src_pad=16),                 # a padded source stride
        Frame(ctx, arena, 16, 3, "xRGB", "ARGB", ST, seed=2, dst_pad=16),                 # a padded destination stride
        Frame(ctx, arena, 5, 3, "BGRx", "BGRA", ST, seed=3),                              # 15 pixels
        Frame(ctx, arena, 16, 3, "xBGR", "ABGR", ST, seed=4, src_off=4),                  # a 4-byte source at +4
        Frame(ctx, arena, 16, 3, "RGBx", "BGRA", ST, seed=5, dst_off=4),                  # a destination at +4
        Frame(ctx, arena, 16, 3, "RGB", "RGBA", ST, seed=6, src_off=1),                   # an RGB source at +1
        Frame(ctx, arena, 64, 5, "BGR", "ARGB", _st(700.0), seed=7),                      # off = -520
        Frame(ctx, arena, 64, 5, "RGBx", "RGBA", _st(-200.0), seed=8),                    # off = 380
        Frame(generic, arena, 64, 48, "RGBx", "ABGR", ST, seed=9),                        # a force-generic member: 12 blocks
        Frame(ctx, arena, 37, 3, "RGB", "BGRA", ST, seed=10, src_pad=1, dst_pad=4),       # odd everything
    ]
    neighbour = Frame(ctx, arena, 64, 48, "RGBx", "RGBA", ST, seed=11)                    # aligned and packed: the vector class
    g = mi355fx.Group(0)
    try:
        assert literal[3].dsrc % 16 == 4 and literal[4].off % 16 == 4 and literal[5].dsrc % 4 == 1
        tk = [f.submit(g) for f in literal]
        for t in tk:
            g.wait_hsvdetect(t)
        assert g.hsvdetect_stats() == (10, 1, 10, 1)                                      # literal jobs alone: one launch
        both = literal[:4] + [neighbour] + literal[4:]
        tk = [f.submit(g) for f in both]                                                  # the same bytes once more
        for t in reversed(tk):
            g.wait_hsvdetect(t)
        assert g.hsvdetect_stats() == (21, 2, 11, 3)                                      # both classes: two launches
        _finish(oracle, arena, both)
    finally:
        _free(g, arena, literal + [neighbour])
        generic.close()


def test_format_matrix_in_three_sets(ctx, oracle):
    """6 input x 4 output formats x three hue_ref classes (0: off = 180; 240: off = -60; 700: literal) at 16 x 3: sets of 32, 32
    and 8. A second round over the same frames gives identical bytes."""
    import mi355fx
    arena = Arena(ctx, 72 * (192 + 64) + 64)
    frames = [Frame(ctx, arena, 16, 3, i, o, _st(hue), seed=100 + k)
              for k, (hue, i, o) in enumerate((hue, i, o) for hue in (0.0, 240.0, 700.0) for i in IN_FMTS for o in OUT_FMTS)]
    g = mi355fx.Group(0)
    try:
        assert len(frames) == 72 and mi355fx.HSVDETECT_SET_MAX == 32
        rounds = []
        for r in range(2):
            tk = []
            for k, f in enumerate(frames):
                tk.append(f.submit(g))
                if k == 63:
                    assert g.hsvdetect_stats()[:3] == (72 * r + 64, 3 * r + 2, 32)       # the 32nd and the 64th submit filled a set
            for t in tk:
                g.wait_hsvdetect(t)
            rounds.append(arena.read()[0])
        # launches follow the classes, by submission order -
        # set 1: 24 x hue 0 + 8 x hue 240 -> vector only (1); set 2: 16 x hue 240 + 16 x hue 700 -> both (2); set 3: 8 x hue 700 -> literal (1)
        assert g.hsvdetect_stats() == (144, 6, 32, 8)
        assert (rounds[0] == rounds[1]).all()
        _finish(oracle, arena, frames)
    finally:
        _free(g, arena, frames)


def test_empty_frames(ctx, oracle):
    import mi355fx
    arena = Arena(ctx, 16 * 1024)
    empty = [Frame(ctx, arena, 0, 3, "RGBx", "RGBA", ST), Frame(ctx, arena, 16, 0, "RGB", "ARGB", ST), Frame(ctx, arena, 0, 0, "BGRx", "BGRA", ST)]
    real = [Frame(ctx, arena, 16, 3, "RGBx", "RGBA", ST, seed=3), Frame(ctx, arena, 5, 3, "BGR", "ABGR", ST, seed=4)]
    g = mi355fx.Group(0)
    try:
        tk = [f.submit(g) for f in empty]
        tk.append(g.submit_hsvdetect(ctx, None, 0, "RGBx", None, 0, "RGBA", 0, 7, ST))   # null pointers are fine without a pixel
        tk.append(g.submit_hsvdetect(ctx, None, 64, "xRGB", None, 64, "ABGR", 16, 0, ST))
        for t in tk:
            g.wait_hsvdetect(t)
        assert g.hsvdetect_stats() == (5, 1, 5, 0)                                        # no job with a pixel: no launch
        assert (arena.read()[0] == arena.sentinel).all()
        tk = [real[0].submit(g), empty[0].submit(g), real[1].submit(g)]
        for t in tk:
            g.wait_hsvdetect(t)
        assert g.hsvdetect_stats() == (8, 2, 5, 2)                                        # a vector and a literal job
        _finish(oracle, arena, empty + real)
    finally:
        _free(g, arena, empty + real)


def test_one_source_three_members(ctx, oracle, synth):
    import mi355fx
    arena = Arena(ctx, 3 * (160 * 90 * 4 + 64) + 64)
    src = synth.smooth_frame(160, 90)
    first = Frame(ctx, arena, 160, 90, "RGBx", "RGBA", ST, host=src)
    frames = [first, Frame(ctx, arena, 160, 90, "RGBx", "ABGR", _st(300.0, hue_var=60.0), share=first),
              Frame(ctx, arena, 160, 90, "RGBx", "BGRA", _st(60.0), share=first)]
    members = [mi355fx.Context(0) for _ in frames]
    g = mi355fx.Group(0)
    try:
        tk = [f.submit(g, c) for f, c in zip(frames, members)]
        for t in tk:
            g.wait_hsvdetect(t)
        assert g.hsvdetect_stats() == (3, 1, 3, 1)
        got = _finish(oracle, arena, frames, members)
        out = [got[f.off: f.off + 160 * 90 * 4] for f in frames]
        assert (out[0] != out[1]).any() and (out[1] != out[2]).any() and (out[0] != out[2]).any()
        # each member's own alpha plane: three different detections of one picture
        al = [out[0][3::4], out[1][0::4], out[2][3::4]]
        assert all(set(np.unique(a).tolist()) == {0, 255} for a in al)
        assert (al[0] != al[1]).any() and (al[1] != al[2]).any() and (al[0] != al[2]).any()
    finally:
        _free(g, arena, frames)
        for c in members:
            c.close()


def test_a_frame_is_read_after_what_its_stream_held(ctx, oracle, synth):
    """Six hsvfilter launches in place, queued asynchronously on the context's stream, then submit at once: the detector sees the
    frame as the last of them leaves it. The queue is tens of microseconds deep when the set is launched on the group's own
    stream, so a set that did not wait for the stream's work would read a frame filtered fewer times."""
    import mi355fx
    w, h = 1920, 1080
    src = synth.smooth_frame(w, h).reshape(-1)
    hs = synth.HSV_SETTINGS["hue90"]
    n_filters = 6
    filtered = src.copy()
    for _ in range(n_filters):
        oracle.hsvfilter(filtered, w, w * 4, 4, 0, False, hs)
    arena = Arena(ctx, w * h * 4 + 128)
    f = Frame(ctx, arena, w, h, "RGBx", "RGBA", ST, host=src)
    g = mi355fx.Group(0)
    try:
        for _ in range(n_filters):
            ctx.hsvfilter_frames_device(f.dsrc, 1, w * h * 4, w, h, w * 4, "RGBx", hs)
        t = f.submit(g)
        g.wait_hsvdetect(t)
        f.host = filtered                                   # what the source holds now
        unfiltered = np.zeros(w * h * 4, np.uint8)
        oracle.hsvdetect(src, w * 4, 4, 0, False, unfiltered, w * 4, False, False, w, ST)
        got = _finish(oracle, arena, [f])
        assert (got[f.off: f.off + w * h * 4] != unfiltered).any()
    finally:
        _free(g, arena, [f])


def test_refusals_and_a_result_is_collected_once(ctx, oracle, synth):
    import mi355fx
    cube = oracle.Cube.parse(synth.cube_text_3d(17))
    sc, of = cube.domain
    ctx.colorlut_load(cube.is3d, cube.size, cube.table, sc, of)
    arena = Arena(ctx, 64 * 1024)
    f = Frame(ctx, arena, 64, 48, "RGBx", "RGBA", ST, seed=21)
    chain_src, chain_dst = ctx.alloc(64 * 48 * 4), ctx.alloc(64 * 48 * 4)     # the chain filters its source in place: not the detector's
    ctx.h2d(chain_src, f.host)
    g = mi355fx.Group(0)
    try:
        d, o = f.dsrc, arena.dg + f.off
        bad = [
            lambda: g.submit_hsvdetect(ctx, d, 256, "RGBA", o, 256, "RGBA", 64, 48, ST),       # RGBA is no input format
            lambda: g.submit_hsvdetect(ctx, d, 256, "RGBx", o, 256, "RGBx", 64, 48, ST),       # RGBx is no output format
            lambda: g.submit_hsvdetect(ctx, d, 256, "RGBx", o, 256, "RGBA", 64, 48, None),     # null settings
            lambda: g.submit_hsvdetect(ctx, d, 252, "RGBx", o, 256, "RGBA", 64, 48, ST),       # strides below the line bytes
            lambda: g.submit_hsvdetect(ctx, d, 256, "RGBx", o, 252, "RGBA", 64, 48, ST),
            lambda: g.submit_hsvdetect(ctx, d, 191, "RGB", o, 256, "RGBA", 64, 48, ST),
            lambda: g.submit_hsvdetect(ctx, None, 256, "RGBx", o, 256, "RGBA", 64, 48, ST),    # null data with a non-empty frame
            lambda: g.submit_hsvdetect(ctx, d, 256, "RGBx", None, 256, "RGBA", 64, 48, ST),
            lambda: g.submit_hsvdetect(ctx, d, 256, "RGBx", o, 256, "RGBA", -1, 48, ST),       # negative sizes
            lambda: g.submit_hsvdetect(ctx, d, 256, "RGBx", o, 256, "RGBA", 64, -1, ST),
            lambda: g.wait_hsvdetect(0),                                                       # unknown tickets
            lambda: g.wait_hsvdetect(12345),
        ]
        t = f.submit(g)
        for call in bad:
            with pytest.raises(mi355fx.Mi355Error) as e:
                call()
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        # the lone entry refuses the same frames with the same status
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.hsvdetect_frames_device(d, 0, 252, "RGBx", arena.dl + f.off, 0, 256, "RGBA", 1, 64, 48, ST)
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.hsvdetect_stats() == (0, 0, 0, 0)                                             # a refused call launches nothing
        # tickets of the other three queues are refused here and stay collectable there
        t_pair = g.submit_compare(ctx, d, d, 256, 64, 48, "RGBA", 5)
        t_cd = g.submit_colordetect(ctx, d, 64 * 48 * 4, "RGBA", 10, 2)
        t_chain = g.submit_chain(ctx, chain_src, chain_dst, 64, 48, 256, "RGBA", synth.HSV_SETTINGS["hue90"])
        for other in (t_pair, t_cd, t_chain):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.wait_hsvdetect(other)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        # ... and the reverse
        for refuse in (g.wait, lambda tt: g.order_after(ctx, tt), g.wait_compare, g.wait_colordetect):
            with pytest.raises(mi355fx.Mi355Error) as e:
                refuse(t)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.hsvdetect_stats() == (0, 0, 0, 0)
        assert g.wait_compare(t_pair)[0] == 0.0
        assert 1 <= len(g.wait_colordetect(t_cd)) <= 2
        g.wait(t_chain)
        assert g.hsvdetect_stats() == (0, 0, 0, 0)                                             # the other queues' launches are theirs
        g.wait_hsvdetect(t)
        assert g.hsvdetect_stats() == (1, 1, 1, 1)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_hsvdetect(t)                                                                # collected
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.hsvdetect_stats() == (1, 1, 1, 1)
        _finish(oracle, arena, [f])
    finally:
        _free(g, arena, [f])
        ctx.free(chain_src)
        ctx.free(chain_dst)


def test_rendezvous_threads_fill_one_set(mi355lib, oracle):
    """Eight instances on eight threads, each submitting its frame and waiting at once (what transform does): with a rendezvous
    of eight the frames of an interval share ONE launch set; a straggler is not waited for longer than the linger."""
    import mi355fx
    n, rounds = 8, 5
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    arena = Arena(ctxs[0], n * (64 * 48 * 4 + 64) + 64)
    frames = [Frame(c, arena, 64, 40 + s, IN4[s % 4], OUT_FMTS[s % 4], _st((120.0, 240.0)[s % 2]), seed=50 + s) for s, c in enumerate(ctxs)]
    g = mi355fx.Group(0)
    g.set_hsvdetect_rendezvous(n, 2_000_000)
    try:
        bar = threading.Barrier(n)
        errors = []

        def element(s):
            try:
                for r in range(rounds):
                    bar.wait()
                    if s == 5:
                        time.sleep(0.01 * r)       # ragged arrival
                    g.wait_hsvdetect(frames[s].submit(g))
            except Exception as e:                 # noqa: BLE001 - told to the main thread
                errors.append(e)
                bar.abort()

        ts = [threading.Thread(target=element, args=(s,)) for s in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert g.hsvdetect_stats() == (n * rounds, rounds, n, rounds)
        # a straggler that never comes: the waiter launches alone after the linger
        g.set_hsvdetect_rendezvous(n, 20_000)
        t0 = time.perf_counter()
        g.wait_hsvdetect(frames[0].submit(g))
        assert 0.015 < time.perf_counter() - t0 < 1.0
        _finish(oracle, arena, frames)
    finally:
        _free(g, arena, frames)
        for c in ctxs:
            c.close()


def test_pairs_colordetect_frames_and_detector_frames_in_one_group(ctx, oracle, synth):
    import mi355fx
    arena = Arena(ctx, 4 * (64 * 48 * 4 + 64) + 64)
    frames = [Frame(ctx, arena, 64, 48, IN_FMTS[s], OUT_FMTS[s], _st((120.0, 240.0)[s % 2]), seed=70 + s) for s in range(4)]
    pic = synth.noise_frame(64, 48, seed=80).reshape(-1)
    d_pic = ctx.alloc(pic.nbytes)
    ctx.h2d(d_pic, pic)
    g = mi355fx.Group(0)
    try:
        palette = ctx.colordetect_frames_device(d_pic, pic.nbytes, pic.nbytes, 1, "RGBA", 1, 4)[0]
        th = [f.submit(g) for f in frames[:2]]
        tp = [g.submit_compare(ctx, d_pic, d_pic, 256, 64, 48, "RGBA", 5)]
        tc = [g.submit_colordetect(ctx, d_pic, pic.nbytes, "RGBA", 1, 4)]
        th += [f.submit(g) for f in frames[2:]]
        tp.append(g.submit_compare(ctx, d_pic, d_pic, 256, 64, 48, "RGBA", 5))
        tc.append(g.submit_colordetect(ctx, d_pic, pic.nbytes, "RGBA", 1, 4))
        assert g.compare_stats() == (0, 0, 0) and g.colordetect_stats() == (0, 0, 0, 0) and g.hsvdetect_stats() == (0, 0, 0, 0)
        g.wait_hsvdetect(th[3])
        assert g.wait_compare(tp[1])[0] == 0.0
        assert g.wait_colordetect(tc[0]) == palette
        g.wait_hsvdetect(th[0])
        assert g.wait_compare(tp[0])[0] == 0.0
        g.wait_hsvdetect(th[2])
        assert g.wait_colordetect(tc[1]) == palette
        g.wait_hsvdetect(th[1])
        assert g.compare_stats() == (2, 1, 2)             # each queue's stats count only its own
        assert g.colordetect_stats() == (2, 1, 2, 2)
        assert g.hsvdetect_stats() == (4, 1, 4, 1)
        _finish(oracle, arena, frames)
    finally:
        _free(g, arena, frames)
        ctx.free(d_pic)


def test_destroy_with_frames_pending(ctx, oracle):
    import mi355fx
    arena = Arena(ctx, 32 * 1024)
    frames = [Frame(ctx, arena, 64, 48, "RGBx", "RGBA", ST, seed=61), Frame(ctx, arena, 33, 21, "RGB", "ABGR", ST, seed=62)]
    g = mi355fx.Group(0)
    try:
        for f in frames:
            f.submit(g)                  # never waited for
        g.close()                        # launches, waits, frees
        g = None
        _finish(oracle, arena, frames)   # the destinations are complete, and the device works: the lone entry runs here
    finally:
        _free(g, arena, frames)
