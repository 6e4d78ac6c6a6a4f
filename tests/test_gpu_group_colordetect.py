"""GPU tests for the colordetect queue of the dispatcher (mi355_group_submit_colordetect / _wait_colordetect): the frames of
INDEPENDENT colordetect instances (one get_palette per frame and element, video/videofx/src/colordetect/imp.rs:57-84) in shared
launch sets - one histogram launch over a job table, one MMCQ launch, one copy. Members differ in plane size, format, quality and
max_colors. The bar: every palette == Context.colordetect_frames_device on the same device bytes AND == the restatement
(tests/colordetect_restate.py), with `==`: the arithmetic is integer only. Parity of the MMCQ contract itself with color-thief stays
unpinned."""
import threading
import time

import numpy as np
import pytest

import colordetect_restate as R

pytestmark = pytest.mark.gpu

_RESTATED = {}


def _want(host, fmt, q, mc):
    """The restatement's palette, computed once per (bytes, settings) of this module."""
    key = (host.tobytes(), fmt, q, mc)
    if key not in _RESTATED:
        _RESTATED[key] = R.get_palette(host, fmt, q, mc)
    return _RESTATED[key]


class Plane:
    """A flat host plane on the device, `offset` bytes into its allocation."""

    def __init__(self, c, host, fmt, q, mc, offset=0):
        self.c, self.fmt, self.q, self.mc = c, fmt, q, mc
        self.host = np.ascontiguousarray(host, dtype=np.uint8).reshape(-1)
        self.n = self.host.nbytes
        self.alloc = c.alloc(self.n + offset + 16)
        self.d = self.alloc + offset
        if self.n:
            c.h2d(self.d, self.host)

    def view(self, n, q=None, mc=None):
        """The first n bytes of the same device bytes as a plane of its own."""
        v = object.__new__(Plane)
        v.c, v.fmt, v.q, v.mc = self.c, self.fmt, q or self.q, mc or self.mc
        v.host, v.n, v.alloc, v.d = self.host[:n], n, None, self.d
        return v

    def submit(self, g, c=None):
        return g.submit_colordetect(c or self.c, self.d, self.n, self.fmt, self.q, self.mc)

    def check(self, got):
        lone = self.c.colordetect_frames_device(self.d, self.n, self.n, 1, self.fmt, self.q, self.mc)[0]
        assert got == lone, (self.fmt, self.q, self.mc, self.n, got, lone)
        assert got == _want(self.host, self.fmt, self.q, self.mc), (self.fmt, self.q, self.mc, self.n)
        return got

    def free(self):
        if self.alloc:
            self.c.free(self.alloc)
            self.alloc = None


def _noise(synth, w, h, ch=4, seed=1):
    return synth.noise_frame(w, h, seed=seed, channels=ch).reshape(-1)


def _tiny(c, synth, s):
    fmt = ("RGBA", "RGB", "BGRA", "BGR", "ARGB")[s % 5]
    ch = R.LAYOUT[fmt][0]
    return Plane(c, _noise(synth, 16, 3 + s % 7, ch, seed=100 + s)[: 16 * (3 + s % 7) * ch - s % 3], fmt, 1 + s % 10, 2 + s % 9)


def test_eight_unlike_members_share_one_set(ctx, synth):
    import mi355fx
    argb = _noise(synth, 64, 48, seed=3).copy()
    argb[0::4] = np.tile(np.array([0, 124, 125, 255, 126, 90], np.uint8), 64 * 48 // 6 + 1)[: 64 * 48]   # alphas on both sides of 125
    planes = [
        Plane(ctx, _noise(synth, 64, 48, seed=1), "RGBA", 10, 2),
        Plane(ctx, _noise(synth, 37, 5, 3, seed=2), "RGB", 1, 5),
        Plane(ctx, argb, "ARGB", 3, 8),
        Plane(ctx, _noise(synth, 50, 20, 3, seed=4), "BGR", 7, 3),
        Plane(ctx, _noise(synth, 64, 48, seed=5), "BGRA", 2, 4, offset=1),          # byte loads beside dword-path neighbours
        Plane(ctx, synth.smooth_frame(192, 128).reshape(-1), "RGBA", 1, 16),         # 24576 samples: two histogram blocks
        Plane(ctx, np.array([7, 9], np.uint8), "RGBA", 1, 2),                        # less than a pixel: no sample
        Plane(ctx, np.full(32 * 32 * 4, 255, np.uint8), "RGBA", 1, 2),               # all white: nothing kept
    ]
    g = mi355fx.Group(0)
    try:
        assert planes[4].d % 4 == 1 and planes[0].d % 4 == 0
        # the plan of this very set: the 192 x 128 plane is the one member with two blocks
        lib = mi355fx.load_library()
        ns = [(p.n // R.LAYOUT[p.fmt][0] + p.q - 1) // p.q for p in planes]
        assert ns[5] == 24576 and ns[6] == 0
        first, blocks, total = _plan(lib, 256, ns)[:3]
        assert blocks == [1, 1, 1, 1, 1, 2, 0, 1] and total == 8
        tk = [p.submit(g) for p in planes]
        assert g.colordetect_stats() == (0, 0, 0, 0)                                # nothing goes out before a wait or a full set
        got = {}
        for i in reversed(range(8)):
            got[i] = planes[i].check(g.wait_colordetect(tk[i]))
        assert got[6] == [] and got[7] == []
        assert all(1 <= len(got[i]) <= planes[i].mc for i in range(6))
        assert g.colordetect_stats() == (8, 1, 8, 2)
    finally:
        g.close()
        for p in planes:
            p.free()


def _plan(lib, n_cu, ns):
    import ctypes as C
    n = len(ns)
    a = (C.c_uint64 * n)(*ns)
    first, blocks, per, total = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint64 * n)(), C.c_uint32(0)
    assert lib.mi355_selftest_colordetect_plan(n_cu, n, a, first, blocks, per, C.byref(total)) == 0
    return list(first), list(blocks), total.value, list(per)


def test_ragged_ends(ctx, synth):
    import mi355fx
    planes = []
    for fmt in ("RGBA", "RGB", "BGRA", "BGR", "ARGB"):
        ch = R.LAYOUT[fmt][0]
        base = Plane(ctx, _noise(synth, 211, 10, ch, seed=ch), fmt, 3, 6)
        planes.append(base)
        for extra in range(1, ch):                                    # 1 .. ch - 1 bytes past the last whole pixel
            planes.append(base.view(ch * 2000 + extra))
        # 3 q + 1 pixels of one colour, the last one another: the last sample IS the last pixel; then the plane one pixel shorter
        for q in (7, 10):
            px = np.zeros((3 * q + 1, ch), np.uint8)
            ri, gi, bi, ai = R.LAYOUT[fmt][1:]
            px[:, ri], px[:, gi], px[:, bi] = 200, 40, 40
            px[-1, ri], px[-1, gi], px[-1, bi] = 10, 220, 10
            if ai is not None:
                px[:, ai] = 255
            whole = Plane(ctx, px.reshape(-1), fmt, q, 2)
            planes += [whole, whole.view(whole.n - ch)]
    g = mi355fx.Group(0)
    try:
        tk = [p.submit(g) for p in planes]
        got = [p.check(g.wait_colordetect(t)) for p, t in zip(planes, tk)]
        k = 0
        for p, pal in zip(planes, got):
            if p.mc == 2 and p.n % R.LAYOUT[p.fmt][0] == 0 and p.n < 200:
                k += 1
                # the plane that ends on the sampled pixel sees the second colour, the shorter one does not
                assert ((12, 220, 12) in pal) == (p.alloc is not None), (p.fmt, p.q, p.n, pal)
        assert k == 20
    finally:
        g.close()
        for p in planes:
            p.free()


def test_more_than_one_set_and_the_scratch_is_zero_again(ctx, synth):
    import mi355fx
    planes = [_tiny(ctx, synth, s) for s in range(40)]
    g = mi355fx.Group(0)
    try:
        rounds = []
        for r in range(2):
            tk = [p.submit(g) for p in planes]
            # the 32nd submit filled a launch set: it has gone out, eight frames are pending
            assert g.colordetect_stats()[:3] == (40 * r + 32, 2 * r + 1, 32)
            rounds.append([p.check(g.wait_colordetect(t)) for p, t in zip(planes, tk)])
        assert rounds[0] == rounds[1]
        assert g.colordetect_stats() == (80, 4, 32, 8)
    finally:
        g.close()
        for p in planes:
            p.free()


def test_sets_without_samples_and_without_kept_samples(ctx, synth):
    """Every job of a set has data_len < ch or nothing kept: all get 0 colours with status OK from ONE launch set. How many kernels
    that set is follows the launch-count rule: a plane shorter than a pixel has no sample, so a set of such planes skips the
    histogram launch (1 kernel); an all-white or all-transparent plane has samples, none of them kept, which only the histogram
    launch can find out (2 kernels). The next set, with real frames, is right: nothing was left behind in the scratch."""
    import mi355fx
    transparent = _noise(synth, 20, 15, seed=9).copy()
    transparent[3::4] = 124
    short = [Plane(ctx, np.array([1, 2, 3], np.uint8), "RGBA", 1, 2), Plane(ctx, np.array([1, 2], np.uint8), "BGR", 5, 9)]
    unkept = [Plane(ctx, np.full(4 * 300, 255, np.uint8), "BGRA", 1, 5), Plane(ctx, transparent, "RGBA", 2, 7), Plane(ctx, np.array([9], np.uint8), "ARGB", 3, 4)]
    real = [Plane(ctx, _noise(synth, 64, 48, seed=11), "RGBA", 1, 8), Plane(ctx, _noise(synth, 31, 17, 3, seed=12), "BGR", 2, 3)]
    g = mi355fx.Group(0)
    try:
        tk = [p.submit(g) for p in short]
        t0 = g.submit_colordetect(ctx, None, 0, "RGB", 10, 2)               # no bytes at all: a null pointer is fine
        assert g.wait_colordetect(t0) == []
        assert [p.check(g.wait_colordetect(t)) for p, t in zip(short, tk)] == [[], []]
        assert g.colordetect_stats() == (3, 1, 3, 1)                        # no job with a sample: the MMCQ launch alone
        tk = [p.submit(g) for p in unkept]
        assert [p.check(g.wait_colordetect(t)) for p, t in zip(unkept, tk)] == [[], [], []]
        assert g.colordetect_stats() == (6, 2, 3, 3)
        tk = [p.submit(g) for p in real]
        assert [len(p.check(g.wait_colordetect(t))) for p, t in zip(real, tk)] == [8, 3]
        assert g.colordetect_stats() == (8, 3, 3, 5)
    finally:
        g.close()
        for p in short + unkept + real:
            p.free()


def test_one_frame_three_members(ctx, synth):
    import mi355fx
    frame = Plane(ctx, synth.smooth_frame(160, 90).reshape(-1), "RGBA", 1, 2)
    members = [(mi355fx.Context(0), frame.view(frame.n, q, mc)) for q, mc in ((1, 2), (10, 2), (4, 255))]
    g = mi355fx.Group(0)
    try:
        tk = [v.submit(g, c) for c, v in members]
        got = [v.check(g.wait_colordetect(t)) for (c, v), t in zip(members, tk)]
        assert got[0] != got[1] and got[1] != got[2] and got[0] != got[2]
        assert len(got[0]) == 2 and len(got[1]) == 2 and len(got[2]) > 100
        assert g.colordetect_stats() == (3, 1, 3, 2)
    finally:
        g.close()
        for c, _ in members:
            c.close()
        frame.free()


def test_a_frame_is_read_after_what_its_stream_held(ctx, synth):
    """hsvfilter in place (asynchronous on the context's stream), then submit at once: the palette is the filtered frame's."""
    import mi355fx
    w, h = 1920, 1080
    src = synth.smooth_frame(w, h).reshape(-1)
    st = synth.HSV_SETTINGS["hue90"]
    ref = Plane(ctx, src, "RGBA", 10, 5)
    ctx.hsvfilter_frames_device(ref.d, 1, w * h * 4, w, h, w * 4, "RGBA", st)
    ctx.synchronize()
    filtered = np.zeros_like(src)
    ctx.d2h(filtered, ref.d)
    ref.host = filtered
    assert _want(filtered, "RGBA", 10, 5) != _want(src, "RGBA", 10, 5)
    work = Plane(ctx, src, "RGBA", 10, 5)
    work.host = filtered
    g = mi355fx.Group(0)
    try:
        ctx.hsvfilter_frames_device(work.d, 1, w * h * 4, w, h, w * 4, "RGBA", st)
        t = work.submit(g)
        got = g.wait_colordetect(t)
        assert got == _want(filtered, "RGBA", 10, 5)
        ref.check(got)
        work.check(got)
    finally:
        g.close()
        ref.free()
        work.free()


def test_refusals_and_a_result_is_collected_once(ctx, synth):
    import mi355fx
    p = Plane(ctx, _noise(synth, 64, 48, seed=21), "RGBA", 2, 6)
    g = mi355fx.Group(0)
    try:
        t = p.submit(g)
        for q, mc in ((0, 2), (11, 2), (10, 1), (10, 256)):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.submit_colordetect(ctx, p.d, p.n, "RGBA", q, mc)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.submit_colordetect(ctx, None, 16, "RGBA", 10, 2)             # a null pointer with bytes
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        for fmt in ("RGBx", "BGRx", "ABGR"):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.submit_colordetect(ctx, p.d, p.n, fmt, 10, 2)
            assert e.value.status == mi355fx.ERR_UNSUPPORTED
        assert g.colordetect_stats() == (0, 0, 0, 0)
        for bad in (0, 12345):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.wait_colordetect(bad)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.colordetect_stats() == (0, 0, 0, 0)                       # a refused wait launches nothing
        # a compare pair's ticket is not a frame's, and stays collectable
        tc = g.submit_compare(ctx, p.d, p.d, 64 * 4, 64, 48, "RGBA", 5)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_colordetect(tc)
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.wait_compare(tc)[0] == 0.0
        # a frame's ticket is neither a pair's nor a filter frame's, and stays collectable
        for refuse in (g.wait_compare, g.wait):
            with pytest.raises(mi355fx.Mi355Error) as e:
                refuse(t)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.colordetect_stats() == (0, 0, 0, 0)
        p.check(g.wait_colordetect(t))
        assert g.colordetect_stats() == (1, 1, 1, 2)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_colordetect(t)                                          # collected
        assert e.value.status == mi355fx.ERR_INVALID_ARG
    finally:
        g.close()
        p.free()


def _cmp_frame(rng, w, h, block=8):
    base = np.kron(rng.integers(0, 256, (h // block, w // block, 4), dtype=np.uint8), np.ones((block, block, 1), np.uint8)).reshape(h, w * 4)
    base[:, 3::4] = 255
    return np.ascontiguousarray(base)


def test_pairs_and_frames_in_one_group(ctx, synth):
    import mi355fx
    rng = np.random.default_rng(31)
    pairs = []   # (w, h, algo, host a, host b, plane a, plane b)
    for w, h, algo in ((128, 96, 5), (640, 480, 4), (128, 96, 5)):
        a = _cmp_frame(rng, w, h)
        b = np.clip(a.astype(int) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
        b[:, 3::4] = 255
        pairs.append((w, h, algo, a, b, Plane(ctx, a, "RGBA", 10, 2), Plane(ctx, b, "RGBA", 10, 2)))
    frames = [Plane(ctx, _noise(synth, 64, 48, seed=40 + s), ("RGBA", "BGRA")[s % 2], 1 + 2 * s, 3 + s) for s in range(4)]
    g = mi355fx.Group(0)
    try:
        tp = [g.submit_compare(ctx, pa.d, pb.d, w * 4, w, h, "RGBA", algo) for (w, h, algo, a, b, pa, pb) in pairs[:2]]
        tf = [p.submit(g) for p in frames[:2]]
        tp.append(g.submit_compare(ctx, pairs[2][5].d, pairs[2][6].d, 128 * 4, 128, 96, "RGBA", 5))
        tf += [p.submit(g) for p in frames[2:]]
        assert g.compare_stats() == (0, 0, 0) and g.colordetect_stats() == (0, 0, 0, 0)
        order = [("f", 3), ("p", 2), ("f", 0), ("p", 0), ("p", 1), ("f", 2), ("f", 1)]
        for kind, i in order:
            if kind == "f":
                frames[i].check(g.wait_colordetect(tf[i]))
                continue
            w, h, algo, a, b, pa, pb = pairs[i]
            dist, h0, h1 = g.wait_compare(tp[i])
            if algo == 5:
                x = ctx.dssim_create_image_device(pa.d, w * 4, w, h, "RGBA")
                assert dist == ctx.dssim_compare_frames_device(x, [pb.d], w * 4, w, h, "RGBA")[0]
                ctx.dssim_free_image(x)
            else:
                assert (h0, h1) == (ctx.videocompare_hash_frame(a, w * 4, w, h, "RGBA"), ctx.videocompare_hash_frame(b, w * 4, w, h, "RGBA"))
                assert dist == float(bin(h0 ^ h1).count("1"))
        assert g.compare_stats() == (3, 2, 2)              # only pairs: a Dssim class of two, a Blockhash class of one
        assert g.colordetect_stats() == (4, 1, 4, 2)       # only frames
    finally:
        g.close()
        for p in frames + [x for pr in pairs for x in pr[5:]]:
            p.free()


def test_rendezvous_threads_fill_one_set(mi355lib, synth):
    """Eight instances on eight threads, each submitting its frame and waiting at once (what transform_ip does): with a rendezvous
    of eight the frames of an interval share ONE launch set; a straggler is not waited for longer than the linger."""
    import mi355fx
    n, rounds = 8, 5
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    planes = [Plane(c, _noise(synth, 64, 40 + s, seed=50 + s), ("RGBA", "ARGB")[s % 2], 1 + s, 2 + 3 * s) for s, c in enumerate(ctxs)]
    g = mi355fx.Group(0)
    g.set_colordetect_rendezvous(n, 2_000_000)
    try:
        got = [[None] * rounds for _ in range(n)]
        bar = threading.Barrier(n)

        def element(s):
            for r in range(rounds):
                bar.wait()
                if s == 5:
                    time.sleep(0.01 * r)       # ragged arrival
                got[s][r] = g.wait_colordetect(planes[s].submit(g))

        ts = [threading.Thread(target=element, args=(s,)) for s in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for s in range(n):
            assert got[s] == [planes[s].check(got[s][0])] * rounds
        assert g.colordetect_stats() == (n * rounds, rounds, n, 2 * rounds)
        # a straggler that never comes: the waiter launches alone after the linger
        g.set_colordetect_rendezvous(n, 20_000)
        t0 = time.perf_counter()
        pal = g.wait_colordetect(planes[0].submit(g))
        assert 0.015 < time.perf_counter() - t0 < 1.0
        planes[0].check(pal)
    finally:
        g.close()
        for p in planes:
            p.free()
        for c in ctxs:
            c.close()


def test_destroy_with_frames_pending(ctx, synth):
    import mi355fx
    planes = [Plane(ctx, _noise(synth, 64, 48, seed=61), "RGBA", 1, 4), Plane(ctx, _noise(synth, 33, 21, 3, seed=62), "RGB", 2, 7)]
    g = mi355fx.Group(0)
    for p in planes:
        p.submit(g)                      # never waited for
    g.close()                            # launches, waits, frees
    for p in planes:
        p.check(ctx.colordetect_frames_device(p.d, p.n, p.n, 1, p.fmt, p.q, p.mc)[0])   # the device is fine, the frames were only read
        p.free()
