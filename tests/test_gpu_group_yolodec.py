"""GPU tests for the decoder queue of the dispatcher (mi355_group_submit_yolodec / _wait_yolodec): the tensors of INDEPENDENT
yolov8tensordec2 / yoloxtensordec instances (one tensor per buffer and element, analytics/analytics/src/yolotensordec/imp.rs:234-422)
in shared launch sets - at most three launches over job tables (yolodec_score_jobs_kernel<V8>, <X>, yolodec_nms_jobs_kernel) and
one download. Members differ in shape, layout, thresholds and output capacity.

The bar for every tensor: the count equal and the records byte-equal (tobytes()) to Context.yolodec_device on the same device
tensor with n_tensors = 1, and yolodec_restate.same_records to yolodec_restate.decode on the host copy (tests/yolodec_cases.py:
the restatement already stands on these inputs)."""
import ctypes as C
import threading

import numpy as np
import pytest

import yolodec_cases as Y
import yolodec_restate as R

pytestmark = pytest.mark.gpu


class Member:
    """One instance's tensor on the device, its settings and its output capacity."""

    def __init__(self, c, case, params=None, max_dets=None, ctx=None):
        self.c, self.case, self.layout, self.F, self.N = c, case, case.layout, case.F, case.N
        self.own = ctx or c
        self.params = case.params if params is None else tuple(float(np.float32(v)) for v in params)
        self.cap = max_dets if max_dets is not None else case.max_dets
        self.d = c.alloc(max(case.data.nbytes, 16))
        if case.data.size:
            c.h2d(self.d, case.data)
        self._want = None

    def want(self):
        if self._want is None:
            self._want = self.case.expected() if self.params == self.case.params else R.decode(self.case.data, self.layout, *np.float32(self.params))
        return self._want

    def submit(self, g):
        return g.submit_yolodec(self.own, self.d, self.layout, self.F, self.N, self.params, self.cap)

    def lone(self):
        got, n = self.own.yolodec_device(self.d, self.F * self.N * 4, 1, self.layout, self.F, self.N, [self.params], self.cap, return_counts=True)
        return got[0], n[0]

    def check(self, result, lone=None):
        got, n = result
        lone_got, lone_n = lone or self.lone()
        want = self.want()
        cap = self.N if self.cap is None else self.cap
        name = self.case.name
        assert n == lone_n == len(want), (name, n, lone_n, len(want))               # the full count, even above the capacity
        assert len(got) == min(n, cap), (name, len(got), n, cap)
        assert got.tobytes() == lone_got.tobytes(), name
        assert R.same_records(got, want[:cap]), name
        return n

    def free(self):
        self.c.free(self.d)


def _settings(k):
    rng = np.random.default_rng(900 + k)
    return (float(rng.uniform(0.3, 0.6)), float(rng.uniform(0.3, 0.6)), float(rng.uniform(0.1, 0.8)))


def _synth(k, layout, F, N, params=None, **kw):
    return Y.Case("m%d_%s_F%d_N%d" % (k, layout, F, N), layout, Y.synth(7000 + k, layout, F, N, frac=0.3), params or _settings(k), **kw)


def _run_set(g, members, reverse=False):
    """Submit all, wait for all, check all; returns the counts."""
    tk = [m.submit(g) for m in members]
    res = {}
    for k in (reversed(range(len(tk))) if reverse else range(len(tk))):
        res[k] = g.wait_yolodec(tk[k])
    return [m.check(res[k]) for k, m in enumerate(members)]


def _free(g, members):
    if g is not None:
        g.close()
    for m in members:
        m.free()


MIXED = [("V8", 84, 256), ("V8", 6, 1), ("X", 85, 512), ("X", 7, 1), ("V8", 133, 1000), ("X", 6, 63), ("V8", 7, 64), ("X", 133, 65), ("V8", 85, 255),
         ("X", 84, 257), ("V8", 6, 512), ("V8", 84, 1), ("X", 85, 256), ("X", 133, 1), ("X", 7, 1000), ("V8", 133, 257), ("X", 84, 255), ("V8", 85, 63),
         ("X", 6, 64), ("V8", 7, 65)]


def test_mixed_shapes_and_layouts_in_one_set(ctx):
    """A job whose N is a multiple of 256 is followed, in its own layout's launch, by a job of one candidate (which survives: its
    thresholds are 0): a block -> job search that is off by one shows there."""
    import mi355fx
    assert {m[1] for m in MIXED} == {6, 7, 84, 85, 133} and {m[2] for m in MIXED} == {1, 63, 64, 65, 255, 256, 257, 512, 1000}
    for layout in ("V8", "X"):
        ns = [m[2] for m in MIXED if m[0] == layout]
        assert any(a % 256 == 0 and b == 1 for a, b in zip(ns, ns[1:]))
    members = [Member(ctx, _synth(k, l, F, N, params=(0.0, 0.0, 0.5) if N == 1 else None)) for k, (l, F, N) in enumerate(MIXED)]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members]
        assert g.yolodec_stats() == (0, 0, 0, 0)                                    # nothing goes out before a wait or a full set
        res = [g.wait_yolodec(t) for t in tk]
        n = len(members)
        assert g.yolodec_stats() == (n, 1, n, 3)
        counts = [m.check(r) for m, r in zip(members, res)]
        assert all(c == 1 for c, m in zip(counts, members) if m.N == 1)
        assert len(set(counts)) > 4 and len({m.params for m in members}) > 10
    finally:
        _free(g, members)


@pytest.mark.parametrize("layout", ["V8", "X"])
def test_one_layout_two_launches_and_a_set_without_candidates(ctx, layout):
    import mi355fx
    F = 12 if layout == "V8" else 13
    members = [Member(ctx, _synth(100 + k, layout, F, N)) for k, N in enumerate((300, 1, 256, 77))]
    empty = [Member(ctx, Y.Case("empty%d" % k, l, np.zeros((f, 0) if l == "V8" else (0, f), np.float32), (0.5, 0.5, 0.5))) for k, (l, f) in
             enumerate((("V8", 6), ("X", 85), ("V8", 1029)))]
    g = mi355fx.Group(0)
    try:
        _run_set(g, members)
        assert g.yolodec_stats() == (4, 1, 4, 2)
        tk = [m.submit(g) for m in empty] + [g.submit_yolodec(ctx, None, layout, 6, 0, (0.5, 0.5, 0.5))]   # a null tensor is fine without a candidate
        assert len(set(tk)) == 4 and all(t > 0 for t in tk)
        for t in tk:
            got, n = g.wait_yolodec(t)
            assert n == 0 and len(got) == 0
        assert g.yolodec_stats() == (8, 2, 4, 2)                                    # no candidate: no launch
        _run_set(g, [members[0], empty[0], members[1]], reverse=True)               # ... and a member without candidates among others
        assert g.yolodec_stats() == (11, 3, 4, 4)
    finally:
        _free(g, members + empty)


def test_lds_and_global_sort_paths_in_one_set(ctx):
    import mi355fx
    cases = Y.group("sort_switch")
    assert sorted(c.N for c in cases) == [4096, 4096, 4097, 4097, 5000, 5000]
    members = [Member(ctx, c) for c in cases[:3]] + [Member(ctx, _synth(200, "X", 9, 1, params=(0.0, 0.0, 0.5)))] + [Member(ctx, c) for c in cases[3:]]
    g = mi355fx.Group(0)
    try:
        counts = _run_set(g, members)
        assert g.yolodec_stats() == (7, 1, 7, 3)
        assert counts[3] == 1 and min(counts[:3] + counts[4:]) > 100
    finally:
        _free(g, members)


def test_survivor_extremes_and_truncation(ctx):
    import mi355fx
    members = [Member(ctx, c) for c in Y.group("survivors") + Y.group("truncation")]
    g = mi355fx.Group(0)
    try:
        counts = _run_set(g, members)
        by_name = {m.case.name: (m, n) for m, n in zip(members, counts)}
        for layout in ("V8", "X"):
            assert by_name["none_" + layout][1] == 0 and by_name["one_" + layout][1] == 1 and by_name["all_" + layout][1] > 50
            for cap in (0, 1, 7):
                m, n = by_name["trunc_%s_%d" % (layout, cap)]
                assert m.cap == cap and n > 7                                       # the full count, above every capacity here
        assert g.yolodec_stats() == (12, 1, 12, 3)
        # max_dets = 0 with null records, through the C entry itself
        m = by_name["trunc_V8_0"][0]
        t = m.submit(g)
        n = C.c_uint32(77)
        assert g.L.mi355_group_wait_yolodec(g.h, t, None, C.byref(n)) == 0 and n.value == by_name["trunc_V8_0"][1]
        # ... and null records with max_dets > 0 are refused; the result stays collectable
        m = by_name["trunc_V8_7"][0]
        t = m.submit(g)
        assert g.L.mi355_group_wait_yolodec(g.h, t, None, C.byref(n)) == mi355fx.ERR_INVALID_ARG
        m.check(g.wait_yolodec(t))
    finally:
        _free(g, members)


def test_known_answers_share_one_set(ctx):
    """kats(), the argmax, tie and cast cases as members of one set: the IoU-exactly-0.5 case and the float below it ride together
    with different iou_threshold."""
    import mi355fx
    kats = Y.kats()
    cases = [k[0] for k in kats] + Y.group("argmax") + Y.group("ties") + Y.group("casts")
    assert {c.params[2] for c in cases} >= {0.5, float(np.float32(Y.IOU_HALF_BELOW))}
    members = [Member(ctx, c) for c in cases]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members]
        res = [g.wait_yolodec(t) for t in reversed(tk)][::-1]
        assert g.yolodec_stats() == (len(members), 1, len(members), 3)
        for m, r in zip(members, res):
            m.check(r)
        for (case, rows, confs), (got, n) in zip(kats, res):
            assert [(int(d["x"]), int(d["y"]), int(d["width"]), int(d["height"]), int(d["class_id"]), int(d["candidate"])) for d in got] == rows, case.name
            assert [d["confidence"].view(np.uint32) for d in got] == [np.float32(c).view(np.uint32) for c in confs], case.name
    finally:
        _free(g, members)


def test_two_sets_and_results_survive_a_growing_slab(ctx):
    """33 submits: sets of 32 and 1. The second set's one member has more records than the whole first set, so every slab grows
    under the first set's uncollected results. Waits come in reverse order."""
    import mi355fx
    small = [Member(ctx, _synth(300 + k, ("V8", "X")[k % 2], (6, 7, 12, 13)[k % 4], (1, 63, 64, 65)[(k // 2) % 4], params=(0.2, 0.2, 0.6))) for k in range(32)]
    big = Member(ctx, Y.group("sort_switch")[2])                                   # 4097 candidates, all surviving
    g = mi355fx.Group(0)
    try:
        assert big.N * 1 > sum(m.N for m in small)
        tk = [m.submit(g) for m in small]
        assert g.yolodec_stats() == (32, 1, 32, 3)                                  # the 32nd submit filled a set
        tb = big.submit(g)
        assert g.yolodec_stats() == (32, 1, 32, 3)
        n_big = big.check(g.wait_yolodec(tb))
        assert g.yolodec_stats() == (33, 2, 32, 5)
        assert n_big * 48 > sum(m.N for m in small) * 48                            # larger than the first set's whole result slab
        res = {k: g.wait_yolodec(tk[k]) for k in reversed(range(32))}
        counts = [m.check(res[k]) for k, m in enumerate(small)]
        assert sum(counts) > 100
        assert g.yolodec_stats() == (33, 2, 32, 5)
    finally:
        _free(g, small + [big])


def test_counters_and_keys_stay_clean_over_intervals(ctx):
    """Big then small then medium on one group: a survivor counter that was not left at zero, or keys of the earlier interval
    read again, change a count."""
    import mi355fx
    sw = Y.group("sort_switch")
    big = [Member(ctx, sw[1]), Member(ctx, sw[3]), Member(ctx, _synth(400, "V8", 20, 1000, params=(0.0, 0.0, 0.5)))]
    small = [Member(ctx, _synth(401, "X", 8, 3)), Member(ctx, Y.kats()[0][0]), Member(ctx, _synth(402, "V8", 8, 5, params=(0.0, 0.0, 0.9))),
             Member(ctx, Y.group("survivors")[0])]
    medium = [Member(ctx, _synth(403 + k, ("X", "V8")[k % 2], 30, 257 + k)) for k in range(5)]
    g = mi355fx.Group(0)
    try:
        lone = {m: m.lone() for m in big + small + medium}
        for members in (big, small, medium, small, big):
            tk = [m.submit(g) for m in members]
            for m, t in zip(members, tk):
                m.check(g.wait_yolodec(t), lone[m])
        assert g.yolodec_stats()[:3] == (19, 5, 5)
    finally:
        _free(g, big + small + medium)


def test_refusals_and_ticket_classes(ctx):
    import mi355fx
    m = Member(ctx, _synth(500, "X", 10, 300))
    pic = np.random.default_rng(3).integers(0, 256, 64 * 48 * 4, dtype=np.uint8)
    d_pic, d_out = ctx.alloc(pic.nbytes), ctx.alloc(pic.nbytes)
    ctx.h2d(d_pic, pic)
    g = mi355fx.Group(0)
    P = (0.5, 0.5, 0.5)
    try:
        bad = [
            (lambda: g.submit_yolodec(ctx, m.d, "X", 5, 300, P), mi355fx.ERR_INVALID_ARG),          # fewer than 6 fields
            (lambda: g.submit_yolodec(ctx, m.d, "X", 1030, 2, P), mi355fx.ERR_UNSUPPORTED),
            (lambda: g.submit_yolodec(ctx, m.d, "X", 10, 65537, P), mi355fx.ERR_UNSUPPORTED),
            (lambda: g.submit_yolodec(ctx, m.d, 2, 10, 300, P), mi355fx.ERR_INVALID_ARG),           # no layout
            (lambda: g.submit_yolodec(ctx, m.d, "X", 10, 300, None), mi355fx.ERR_INVALID_ARG),      # null settings
            (lambda: g.submit_yolodec(ctx, m.d + 2, "X", 10, 300, P), mi355fx.ERR_INVALID_ARG),     # misaligned
            (lambda: g.submit_yolodec(ctx, None, "X", 10, 300, P), mi355fx.ERR_INVALID_ARG),        # null tensor with candidates
            (lambda: g.submit_yolodec(None, m.d, "X", 10, 300, P), mi355fx.ERR_INVALID_ARG),        # null context
            (lambda: g.wait_yolodec(0), mi355fx.ERR_INVALID_ARG),                                   # unknown tickets
            (lambda: g.wait_yolodec(12345), mi355fx.ERR_INVALID_ARG),
        ]
        for call, status in bad:
            with pytest.raises(mi355fx.Mi355Error) as e:
                call()
            assert e.value.status == status
        assert g.L.mi355_group_submit_yolodec(g.h, ctx.h, m.d, 1, 10, 300, C.byref(mi355fx.YoloParams(*P)), 300, None) == mi355fx.ERR_INVALID_ARG   # null ticket
        # the lone entry refuses the same shapes with the same status
        for F, N, status in ((5, 300, mi355fx.ERR_INVALID_ARG), (10, 65537, mi355fx.ERR_UNSUPPORTED)):
            with pytest.raises(mi355fx.Mi355Error) as e:
                ctx.yolodec_device(m.d, F * N * 4, 1, "X", F, N, [P])
            assert e.value.status == status
        assert g.yolodec_stats() == (0, 0, 0, 0)
        g.flush()
        assert g.yolodec_stats() == (0, 0, 0, 0)                                    # a refused submit queued nothing
        t = m.submit(g)
        # tickets of the other queues are refused here and stay collectable there
        t_pair = g.submit_compare(ctx, d_pic, d_pic, 256, 64, 48, "RGBA", 5)
        t_cd = g.submit_colordetect(ctx, d_pic, pic.nbytes, "RGBA", 10, 2)
        t_hd = g.submit_hsvdetect(ctx, d_pic, 256, "RGBx", d_out, 256, "RGBA", 64, 48, (120.0, 40.0, 0.8, 0.5, 0.7, 0.6))
        for other in (t_pair, t_cd, t_hd):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.wait_yolodec(other)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        # ... and the reverse
        for refuse in (g.wait, lambda tt: g.order_after(ctx, tt), g.wait_compare, g.wait_colordetect, g.wait_hsvdetect):
            with pytest.raises(mi355fx.Mi355Error) as e:
                refuse(t)
            assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.yolodec_stats() == (0, 0, 0, 0)
        assert g.wait_compare(t_pair)[0] == 0.0
        assert 1 <= len(g.wait_colordetect(t_cd)) <= 2
        g.wait_hsvdetect(t_hd)
        assert g.yolodec_stats() == (0, 0, 0, 0)                                    # the other queues' launches are theirs
        m.check(g.wait_yolodec(t))                                                  # the first valid submit after the refusals is right
        assert g.yolodec_stats() == (1, 1, 1, 2)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_yolodec(t)                                                       # collected
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        assert g.yolodec_stats() == (1, 1, 1, 2)
    finally:
        _free(g, [m])
        ctx.free(d_pic)
        ctx.free(d_out)


def test_a_tensor_is_read_after_what_its_stream_held(ctx):
    """The tensor is written by a device copy on the member's stream immediately before the submit, behind four 64 MiB copies that
    keep the stream busy, with no synchronisation: the set, on the queue's own stream, must wait for it."""
    import mi355fx
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3
    real = _synth(600, "V8", 84, 1000, params=(0.4, 0.45, 0.45))
    decoy = Y.Case("decoy", "V8", Y.synth(7601, "V8", 84, 1000, frac=0.3), real.params)
    m = Member(ctx, decoy)                                                          # the device tensor holds the decoy for now
    stage = ctx.alloc(real.data.nbytes)
    ctx.h2d(stage, real.data)
    filler = 64 << 20
    a, b = ctx.alloc(filler), ctx.alloc(filler)
    g = mi355fx.Group(0)
    try:
        old = m.lone()
        assert old[1] == len(decoy.expected())
        for _ in range(4):
            assert hip.hipMemcpyAsync(b, a, filler, D2D, ctx.stream) == 0
        assert hip.hipMemcpyAsync(m.d, stage, real.data.nbytes, D2D, ctx.stream) == 0
        t = m.submit(g)
        got = g.wait_yolodec(t)
        m.case, m._want = real, None                                                # what the tensor holds now
        m.check(got)
        assert got[0].tobytes() != old[0].tobytes()
    finally:
        _free(g, [m])
        for p in (stage, a, b):
            ctx.free(p)


def test_rendezvous_threads(mi355lib):
    """Eight instances on eight threads x 20 intervals, each with its own context, shape and layout, submitting and waiting at once
    (what transform_ip does); rendezvous 8 with a 2 ms linger. One thread sits out every third interval."""
    import mi355fx
    n, rounds = 8, 20
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    members = [Member(ctxs[0], _synth(700 + s, ("V8", "X")[s % 2], (84, 85, 6, 7, 20, 21, 133, 12)[s], (300, 257, 1, 1000, 64, 512, 63, 255)[s]), ctx=c)
               for s, c in enumerate(ctxs)]
    g = mi355fx.Group(0)
    g.set_yolodec_rendezvous(n, 2000)
    try:
        lone = [m.lone() for m in members]
        for m, l in zip(members, lone):
            m.check(l, l)                                                           # the lone answers against the restatement, once
        bar = threading.Barrier(n)
        errors, seen = [], [0] * n

        def element(s):
            try:
                for r in range(rounds):
                    bar.wait()
                    if s == 5 and r % 3 == 2:
                        continue
                    got, cnt = g.wait_yolodec(members[s].submit(g))
                    assert cnt == lone[s][1] and got.tobytes() == lone[s][0].tobytes(), (s, r)
                    seen[s] += 1
            except Exception as e:                 # noqa: BLE001 - told to the main thread
                errors.append(e)
                bar.abort()

        ts = [threading.Thread(target=element, args=(s,)) for s in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        total = n * rounds - len([r for r in range(rounds) if r % 3 == 2])
        st = g.yolodec_stats()
        assert sum(seen) == total == st[0] and st[2] <= n and rounds <= st[1] <= total and st[3] <= 3 * st[1]
    finally:
        _free(g, members)
        for c in ctxs:
            c.close()


def test_flush_wait_all_and_destroy_cover_the_queue(ctx):
    import mi355fx
    members = [Member(ctx, _synth(800 + k, ("V8", "X")[k % 2], 15, 200 + 57 * k)) for k in range(4)]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members[:2]]
        g.flush()
        assert g.yolodec_stats() == (2, 1, 2, 3)                                    # flush launches the queue
        tk += [m.submit(g) for m in members[2:]]
        g.wait_all()                                                                # launches and waits; results stay collectable
        assert g.yolodec_stats() == (4, 2, 2, 6)
        for m, t in zip(members, tk):
            m.check(g.wait_yolodec(t))
        for m in members:
            m.submit(g)                                                             # two launched and never waited for, two pending
            if m is members[1]:
                g.flush()
        g.close()                                                                   # launches, waits, frees: does not hang
        g = None
        for m in members:
            m.check(m.lone())                                                       # the device works
    finally:
        _free(g, members)


def test_realistic_shapes_in_one_set(ctx):
    """8400 x 84 (V8) and 8400 x 85 (X), eight members each, one set, once."""
    import mi355fx
    members = [Member(ctx, Y.realistic(("V8", "X")[k % 2], seed=k // 2), max_dets=128) for k in range(16)]
    g = mi355fx.Group(0)
    try:
        counts = _run_set(g, members)
        assert g.yolodec_stats() == (16, 1, 16, 3)
        assert all(10 < c <= 128 for c in counts), counts
    finally:
        _free(g, members)
