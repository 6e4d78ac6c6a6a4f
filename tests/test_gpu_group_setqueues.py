"""The set-queue protocol of the dispatcher (csrc/group.hip, SetQueue<Kind>) for five of its kinds - colordetect, hsvdetector,
hsvfilter, decoder and the videocompare pairs (the hand decoder's queue is the subject of its own file) - one script per path the per-queue files leave open,
each run for every kind through a small adaptor: sets collected out of order (Q1), more sets in flight than the blocks of first
use (Q2), flush (Q3), a wait for a ticket in the middle of the pending list (Q4) and all kinds in one group (Q5). One thread, no
rendezvous: every step is deterministic. The compare queue is the kind with lanes: a launch set goes out as up to eight parts on
eight streams, and what Q1 collects in reverse it collects per lane.

The bar is `==` against the lone entry on the same Context and the same device bytes (Context.colordetect_frames_device,
Context.hsvdetect_frames_device, Context.hsvfilter_frames_device, Context.yolodec_device with one tensor, Context.dssim_create_image_device +
dssim_compare_frames_device), computed once per item of this module. Items differ by seed, so a result handed to the wrong ticket
is seen. The stats' launches column follows each kind's launch rule: colordetect one histogram and one MMCQ launch per set;
hsvdetector and hsvfilter one launch for a set of vector-class frames (all frames here are packed and aligned, the detector's on the
dial, the filter's with finite settings and a hue shift within +-360); decoder one score
launch per layout present and one NMS launch; the compare queue reports none."""
import numpy as np
import pytest

import yolodec_cases as Y

pytestmark = pytest.mark.gpu

SET_MAX = 32
N_ITEMS = 5 * SET_MAX
W, H = 64, 48                                  # the smallest frames of the per-queue files


class Colordetect:
    name = "colordetect"

    def __init__(self, c):
        self.c, self.items, self._lone = c, [], {}
        for i in range(N_ITEMS):
            rng = np.random.default_rng(1000 + i)
            fmt = ("RGBA", "BGRA", "ARGB")[i % 3]
            px = np.clip(rng.integers(0, 256, 3) + rng.integers(-70, 71, (W * H, 3)), 0, 255).astype(np.uint8)   # a colour of its own, with noise
            host = np.full((W * H, 4), 255, np.uint8)                                 # opaque
            first = 1 if fmt == "ARGB" else 0
            host[:, first: first + 3] = px
            host = host.reshape(-1)
            d = c.alloc(host.nbytes)
            c.h2d(d, host)
            self.items.append((d, host.nbytes, fmt, 1 + i % 10, 2 + i % 7))

    def reset(self):
        pass

    def submit(self, g, i):
        d, n, fmt, q, mc = self.items[i]
        return g.submit_colordetect(self.c, d, n, fmt, q, mc)

    def wait(self, g, i, ticket):
        return g.wait_colordetect(ticket)

    def lone(self, i):
        if i not in self._lone:
            d, n, fmt, q, mc = self.items[i]
            self._lone[i] = self.c.colordetect_frames_device(d, n, n, 1, fmt, q, mc)[0]
        return self._lone[i]

    def key(self, result):
        return tuple(result)

    def stats(self, g):
        return g.colordetect_stats()

    def launches(self, idx):
        return 2

    def free(self):
        for it in self.items:
            self.c.free(it[0])


class Hsvdetect:
    """The result of a frame is what its destination holds after the wait. The group writes into one arena, the lone entry into a
    second one prepared alike; reset() puts the sentinel back into the group's arena, so a frame that was not written is seen."""
    name = "hsvdetect"
    IN, OUT = ("RGBx", "xRGB", "BGRx", "xBGR"), ("RGBA", "ARGB", "BGRA", "ABGR")

    def __init__(self, c):
        self.c, self._lone = c, None
        self.fb = W * H * 4
        n = N_ITEMS * self.fb
        self.src = np.random.default_rng(2000).integers(0, 256, n, dtype=np.uint8)
        self.sentinel = ((np.arange(n, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)
        self.d_src, self.dg, self.dl = c.alloc(n), c.alloc(n), c.alloc(n)
        c.h2d(self.d_src, self.src)
        c.h2d(self.dl, self.sentinel)
        self.reset()

    def _args(self, i, dst):
        st = ((120.0, 240.0, 0.0)[i % 3], 40.0 + i % 5, 0.8, 0.5, 0.7, 0.6)
        return self.d_src + i * self.fb, W * 4, self.IN[i % 4], dst + i * self.fb, W * 4, self.OUT[(i // 4) % 4], st

    def reset(self):
        self.c.h2d(self.dg, self.sentinel)

    def submit(self, g, i):
        s, ss, sf, d, ds, df, st = self._args(i, self.dg)
        return g.submit_hsvdetect(self.c, s, ss, sf, d, ds, df, W, H, st)

    def wait(self, g, i, ticket):
        g.wait_hsvdetect(ticket)
        got = np.zeros(self.fb, np.uint8)
        self.c.d2h(got, self.dg + i * self.fb)
        return got.tobytes()

    def lone(self, i):
        if self._lone is None:
            for k in range(N_ITEMS):
                s, ss, sf, d, ds, df, st = self._args(k, self.dl)
                self.c.hsvdetect_frames_device(s, 0, ss, sf, d, 0, ds, df, 1, W, H, st)
            self.c.synchronize()
            all_ = np.zeros(N_ITEMS * self.fb, np.uint8)
            self.c.d2h(all_, self.dl)
            assert (all_ != self.sentinel).any()
            self._lone = [all_[k * self.fb: (k + 1) * self.fb].tobytes() for k in range(N_ITEMS)]
        return self._lone[i]

    def key(self, result):
        return result

    def stats(self, g):
        return g.hsvdetect_stats()

    def launches(self, idx):
        return 1

    def free(self):
        for p in (self.d_src, self.dg, self.dl):
            self.c.free(p)


class Hsvfilter:
    """The result of a frame is what its slice holds after the wait: frames are filtered IN PLACE, each in a slice of its own of one
    arena, so no two overlap. reset() puts the source bytes back into the group's arena; the lone entry filters a second arena that
    holds the same bytes. The 3-byte formats fill the first three quarters of their slice; the rest must come back untouched."""
    name = "hsvfilter"
    FMTS = ("RGBx", "xRGB", "BGRx", "xBGR", "RGBA", "ARGB", "BGRA", "ABGR", "RGB", "BGR")

    def __init__(self, c):
        self.c, self._lone = c, None
        self.fb = W * H * 4
        n = N_ITEMS * self.fb
        self.src = np.random.default_rng(5000).integers(0, 256, n, dtype=np.uint8)
        self.dg, self.dl = c.alloc(n), c.alloc(n)
        c.h2d(self.dl, self.src)
        self.reset()

    def _args(self, i, arena):
        fmt = self.FMTS[i % 10]
        ident = i % 4 == 0                                                            # identity saturation / value: the other variants
        st = ((0.0, 90.0, -120.0, 360.0, -360.0, 45.5, -0.25)[i % 7],) + ((1.0, 0.0, 1.0, 0.0) if ident else
                                                                           (0.5 + 0.25 * (i % 5), 0.1 * (i % 3 - 1), 0.6 + 0.2 * (i % 3), 0.05 * (i % 4 - 1)))
        return arena + i * self.fb, W, H, W * (3 if fmt in ("RGB", "BGR") else 4), fmt, st

    def reset(self):
        self.c.h2d(self.dg, self.src)

    def submit(self, g, i):
        return g.submit_hsvfilter(self.c, *self._args(i, self.dg))

    def wait(self, g, i, ticket):
        g.wait_hsvfilter(ticket)
        got = np.zeros(self.fb, np.uint8)
        self.c.d2h(got, self.dg + i * self.fb)
        return got.tobytes()

    def lone(self, i):
        if self._lone is None:
            for k in range(N_ITEMS):
                d, w, h, stride, fmt, st = self._args(k, self.dl)
                self.c.hsvfilter_frames_device(d, 1, 0, w, h, stride, fmt, st)
            self.c.synchronize()
            all_ = np.zeros(N_ITEMS * self.fb, np.uint8)
            self.c.d2h(all_, self.dl)
            assert (all_ != self.src).any()
            self._lone = [all_[k * self.fb: (k + 1) * self.fb].tobytes() for k in range(N_ITEMS)]
        return self._lone[i]

    def key(self, result):
        return result

    def stats(self, g):
        return g.hsvfilter_stats()

    def launches(self, idx):
        return 1

    def free(self):
        for p in (self.dg, self.dl):
            self.c.free(p)


class Yolodec:
    name = "yolodec"

    def __init__(self, c):
        self.c, self.items, self._lone = c, [], {}
        for i in range(N_ITEMS):
            layout = ("V8", "X")[i % 2]
            F, N = (12, 13)[i % 2], (63, 64, 65, 33)[(i // 2) % 4]
            data = np.ascontiguousarray(Y.synth(3000 + i, layout, F, N, frac=0.3), np.float32)
            d = c.alloc(data.nbytes)
            c.h2d(d, data)
            self.items.append((d, layout, F, N, (0.2, 0.2, 0.6), (None, 5)[i % 5 == 4]))      # every fifth with a capacity below its count

    def reset(self):
        pass

    def submit(self, g, i):
        d, layout, F, N, P, cap = self.items[i]
        return g.submit_yolodec(self.c, d, layout, F, N, P, cap)

    def wait(self, g, i, ticket):
        got, n = g.wait_yolodec(ticket)
        return got.tobytes(), n

    def lone(self, i):
        if i not in self._lone:
            d, layout, F, N, P, cap = self.items[i]
            got, n = self.c.yolodec_device(d, F * N * 4, 1, layout, F, N, [P], cap, return_counts=True)
            self._lone[i] = (got[0].tobytes(), n[0])
        return self._lone[i]

    def key(self, result):
        return result[0]

    def stats(self, g):
        return g.yolodec_stats()

    def launches(self, idx):
        return len({self.items[i][1] for i in idx}) + 1

    def free(self):
        for it in self.items:
            self.c.free(it[0])


class Compare:
    """Dssim pairs of one class (one size, one format, the exact form), so that launch sets are the contiguous runs of the pending
    list the scripts' stats expect; classes are test_gpu_group_compare.py's subject. A set's pairs go out over the group's default
    eight lanes, so a script that collects out of order collects per lane. The compare queue reports no launch column:
    compare_stats() has three figures, shown here with a launch count of 0."""
    name = "compare"

    def __init__(self, c):
        self.c, self.items, self._lone = c, [], {}
        for i in range(N_ITEMS):
            rng = np.random.default_rng(4000 + i)
            a = np.kron(rng.integers(0, 256, (H // 8, W // 8, 4), dtype=np.uint8), np.ones((8, 8, 1), np.uint8)).reshape(H, W * 4)   # a frame of its own ...
            amp = 2 + 3 * (i % 29)
            b = np.clip(a.astype(int) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)                                 # ... and a noisy copy
            a[:, 3::4] = b[:, 3::4] = 255
            pair = []
            for host in (a, b):
                d = c.alloc(host.nbytes)
                c.h2d(d, np.ascontiguousarray(host).reshape(-1))
                pair.append(d)
            self.items.append(tuple(pair))

    def reset(self):
        pass

    def submit(self, g, i):
        d_ref, d_frame = self.items[i]
        return g.submit_compare(self.c, d_ref, d_frame, W * 4, W, H, "RGBA", 5)

    def wait(self, g, i, ticket):
        return g.wait_compare(ticket)[0]

    def lone(self, i):
        if i not in self._lone:
            d_ref, d_frame = self.items[i]
            x = self.c.dssim_create_image_device(d_ref, W * 4, W, H)
            self._lone[i] = self.c.dssim_compare_frames_device(x, [d_frame], W * 4, W, H)[0]
            self.c.dssim_free_image(x)
        return self._lone[i]

    def key(self, result):
        return result

    def stats(self, g):
        return g.compare_stats() + (0,)

    def launches(self, idx):
        return 0

    def free(self):
        for it in self.items:
            self.c.free(it[0])
            self.c.free(it[1])


KINDS = {"colordetect": Colordetect, "hsvdetect": Hsvdetect, "hsvfilter": Hsvfilter, "yolodec": Yolodec, "compare": Compare}


@pytest.fixture(scope="module")
def pools(mi355lib):
    """One context, and per kind its items on the device and their lone values: built at first use, once for the module."""
    import mi355fx
    c = mi355fx.Context(0)
    made = {}

    def get(kind):
        if kind not in made:
            a = made[kind] = KINDS[kind](c)
            lone = [a.lone(i) for i in range(N_ITEMS)]
            assert len({a.key(v) for v in lone}) > N_ITEMS * 9 // 10, kind           # distinct by seed ...
            if kind == "colordetect":
                assert all(1 <= len(v) <= a.items[i][4] for i, v in enumerate(lone))   # ... and not trivial
            if kind == "yolodec":
                assert sum(v[1] > 0 for v in lone) > N_ITEMS * 9 // 10 and any(v[1] > 5 for i, v in enumerate(lone) if i % 5 == 4)
        a = made[kind]
        a.reset()
        return a

    yield get
    for a in made.values():
        a.free()
    c.close()


def _sets_launches(a, n):
    """The launches of items 0 .. n-1 as consecutive full sets."""
    return sum(a.launches(range(k, min(k + SET_MAX, n))) for k in range(0, n, SET_MAX))


def _collected(g, a, i, ticket):
    import mi355fx
    with pytest.raises(mi355fx.Mi355Error) as e:
        a.wait(g, i, ticket)
    assert e.value.status == mi355fx.ERR_INVALID_ARG


@pytest.mark.parametrize("kind", list(KINDS))
def test_q1_sets_collected_out_of_order(pools, kind):
    import mi355fx
    a = pools(kind)
    n = 2 * SET_MAX + 1
    g = mi355fx.Group(0)
    try:
        tk = [a.submit(g, i) for i in range(n)]
        assert len(set(tk)) == n
        two = _sets_launches(a, 2 * SET_MAX)
        assert a.stats(g) == (2 * SET_MAX, 2, SET_MAX, two)                           # two full flushes, one item pending
        assert a.wait(g, n - 1, tk[n - 1]) == a.lone(n - 1)                           # launches the third set alone
        end = (n, 3, SET_MAX, two + a.launches([n - 1]))
        assert a.stats(g) == end
        for i in reversed(range(n - 1)):
            assert a.wait(g, i, tk[i]) == a.lone(i), (kind, i)
        assert a.stats(g) == end
        for i in (0, SET_MAX - 1, SET_MAX, n - 1):
            _collected(g, a, i, tk[i])
        assert a.stats(g) == end
    finally:
        g.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_q2_more_sets_in_flight_than_first_use_blocks(pools, kind):
    import mi355fx
    a = pools(kind)
    n = 5 * SET_MAX
    g = mi355fx.Group(0)
    try:
        tk = [a.submit(g, i) for i in range(n)]
        launched = (n, 5, SET_MAX, _sets_launches(a, n))
        # five sets launched back to back with no wait in between. How many are in flight at once is the device's pace: a submit
        # collects sets that have already finished, so the pool's growth past its first-use blocks is reached when the device is
        # behind, and block reuse when it keeps up - the results must be right either way
        assert a.stats(g) == launched
        g.wait_all()
        assert a.stats(g) == launched
        for i in range(n):
            assert a.wait(g, i, tk[i]) == a.lone(i), (kind, i)
        assert a.stats(g) == launched                                                 # a wait after wait_all launches nothing
    finally:
        g.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_q3_flush(pools, kind):
    import mi355fx
    a = pools(kind)
    g = mi355fx.Group(0)
    try:
        tk = [a.submit(g, i) for i in range(3)]
        assert a.stats(g) == (0, 0, 0, 0)
        g.flush()
        one = (3, 1, 3, a.launches(range(3)))
        assert a.stats(g) == one
        for i in range(3):
            assert a.wait(g, i, tk[i]) == a.lone(i), (kind, i)
        assert a.stats(g) == one
    finally:
        g.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_q4_wait_for_a_ticket_in_the_middle_of_the_pending_list(pools, kind):
    import mi355fx
    a = pools(kind)
    n = SET_MAX + 3
    g = mi355fx.Group(0)
    try:
        tk = [a.submit(g, i) for i in range(n)]
        full = a.launches(range(SET_MAX))
        assert a.stats(g) == (SET_MAX, 1, SET_MAX, full)                              # one full set, three pending
        mid = SET_MAX + 1
        assert a.wait(g, mid, tk[mid]) == a.lone(mid)
        # the three are ONE set: sets take pending items in submission order, and `until` stops after the set that carries it
        two = (n, 2, SET_MAX, full + a.launches(range(SET_MAX, n)))
        assert a.stats(g) == two
        for i in (n - 1, SET_MAX):
            assert a.wait(g, i, tk[i]) == a.lone(i), (kind, i)
        for i in range(SET_MAX):
            assert a.wait(g, i, tk[i]) == a.lone(i), (kind, i)
        assert a.stats(g) == two
        _collected(g, a, mid, tk[mid])
    finally:
        g.close()


def test_q5_all_kinds_in_one_group(pools):
    import mi355fx
    kinds = [pools(k) for k in KINDS]
    nk = len(kinds)
    n = SET_MAX + 1                                                                   # two sets each: a full one and one of one
    g = mi355fx.Group(0)
    try:
        tk = {}
        for i in range(n):
            for a in kinds:                                                           # interleaved: cd, hd, hf, yd, cmp, cd, hd, hf, yd, cmp, ...
                tk[a.name, i] = a.submit(g, i)
        assert len(set(tk.values())) == nk * n                                        # one ticket sequence
        for a in kinds:
            assert a.stats(g) == (SET_MAX, 1, SET_MAX, a.launches(range(SET_MAX)))
        # items from the last to the first, the kinds rotating: never the order of submission
        for i in reversed(range(n)):
            for a in (kinds[(i + 2 + j) % nk] for j in range(nk)):
                assert a.wait(g, i, tk[a.name, i]) == a.lone(i), (a.name, i)
        for a in kinds:
            assert a.stats(g) == (n, 2, SET_MAX, a.launches(range(SET_MAX)) + a.launches([SET_MAX])), a.name   # each queue counts only its own
        # every ticket is its own queue's alone, and collected once
        for a, other in zip(kinds, kinds[1:] + kinds[:1]):
            _collected(g, other, 0, tk[a.name, 0])
            _collected(g, a, 0, tk[a.name, 0])
    finally:
        g.close()
