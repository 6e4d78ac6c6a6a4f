"""GPU tests for the hand-decoder queue of the dispatcher (mi355_group_submit_handdec_palm / _landmarks / _wait_handdec): the tensors
of INDEPENDENT handdetectiontensordec / handlandmarktensordec instances (one tensor per buffer and element,
analytics/analytics/src/hand/handdetectiontensordec/imp.rs, hand/handlandmarktensordec/imp.rs: transform_ip) in shared launch sets -
at most two launches over job tables (handdec_palm_jobs_kernel, handdec_landmark_jobs_kernel), no upload and one download. Members
differ in decoder, shape, scores and settings.

The bar for every ticket: the count equal and the written records byte-equal (tobytes()) to Context.handdec_palm_device /
handdec_landmarks_device on the same device tensor with n_tensors = 1, and equal to case.expected() (tests/handdec_restate.py) under
the comparison of tests/test_gpu_handdec.py: f32 fields NaN == NaN, everything else by bits. Every device tensor sits in a larger
allocation with poison behind it."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import handdec_cases as H
import handdec_group_members as M
import handdec_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = np.float32(7e30)   # behind every tensor: as a score it would survive any threshold
FILL = 0xA5                 # the byte the caller's result arrays hold before a wait


def _why(got, want):
    return "\ngot  %r\nwant %r" % (got, want)


def _check_palm(got, case, what):
    want = case.expected()
    assert len(got) == len(want), (case.name, what, len(got), len(want))
    assert R.same_records(got, want), (case.name, what, _why(got, want))


def _check_landmarks(got, case, what):
    want_d, want_k = case.expected()
    assert len(got[0]) == len(want_d) and len(got[1]) == len(want_d), (case.name, what, len(got[0]), len(want_d))
    assert R.same_records(got[0], want_d), (case.name, what, _why(got[0], want_d))
    assert R.same_records(got[1], want_k), (case.name, what, _why(got[1], want_k))


def _upload(c, a):
    """the array at the start of a larger allocation, poison behind it"""
    buf = np.full(a.size + 64, POISON, np.float32)
    buf[:a.size] = a.reshape(-1)
    d = c.alloc(buf.nbytes)
    c.h2d(d, buf)
    return d


class Member:
    """One instance's tensor (and scores) on the device and its settings."""

    def __init__(self, c, case, ctx=None):
        self.c, self.case, self.own = c, case, ctx or c
        self.palm = isinstance(case, H.PalmCase)
        self.rows = case.N if self.palm else case.H
        self.d = _upload(c, case.data)
        self.ds, self.ns = None, 0
        if not self.palm and case.scores is not None and len(case.scores):
            self.ds, self.ns = _upload(c, case.scores), len(case.scores)

    @property
    def params(self):
        return H.flat_params(self.case.params)

    def submit(self, g):
        if self.palm:
            return g.submit_handdec_palm(self.own, self.d, self.rows, self.params)
        return g.submit_handdec_landmarks(self.own, self.d, self.rows, self.case.D, self.params, self.ds, self.ns)

    def lone(self):
        if self.palm:
            return self.own.handdec_palm_device(self.d, self.rows * 32, 1, self.rows, [self.params])[0]
        return self.own.handdec_landmarks_device(self.d, self.rows * 21 * self.case.D * 4, 1, self.rows, self.case.D, [self.params], self.ds, self.ns * 4, self.ns)[0]

    def check(self, got, lone=None):
        lone = self.lone() if lone is None else lone
        name = self.case.name
        if self.palm:
            assert len(got) == len(lone) and got.tobytes() == lone.tobytes(), (name, _why(got, lone))
            _check_palm(got, self.case, "set")
            return len(got)
        assert len(got[0]) == len(got[1]) == len(lone[0]), name
        assert got[0].tobytes() == lone[0].tobytes() and got[1].tobytes() == lone[1].tobytes(), (name, _why(got, lone))
        _check_landmarks(got, self.case, "set")
        return len(got[0])

    def free(self):
        self.c.free(self.d)
        if self.ds is not None:
            self.c.free(self.ds)


def _raw_wait(g, ticket, null_kps=False):
    """mi355_group_wait_handdec itself, into arrays pre-filled with FILL -> (status, dets, kps, n); the arrays whole"""
    import mi355fx
    dets, kps = np.zeros(mi355fx.HAND_MAX, mi355fx.HAND_DET), np.zeros(mi355fx.HAND_MAX, mi355fx.HAND_KP)
    dets.view(np.uint8)[:] = FILL
    kps.view(np.uint8)[:] = FILL
    n = C.c_uint32(77)
    rc = g.L.mi355_group_wait_handdec(g.h, ticket, dets.ctypes.data, None if null_kps else kps.ctypes.data, C.byref(n))
    return rc, dets, kps, n.value


def _run_set(g, members, reverse=False, lone=None):
    """Submit all, wait for all, check all; returns the counts."""
    order = list(reversed(range(len(members)))) if reverse else list(range(len(members)))
    tk = {k: members[k].submit(g) for k in order}
    res = {k: g.wait_handdec(tk[k]) for k in order}
    return [m.check(res[k], None if lone is None else lone[m]) for k, m in enumerate(members)]


def _free(g, members):
    if g is not None:
        g.close()
    for m in members:
        m.free()


def test_mixed_decoders_shapes_and_settings_in_one_set(ctx):
    import mi355fx
    members = [Member(ctx, c) for c in M.mixed_cases()]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members]
        assert g.handdec_stats() == (0, 0, 0, 0)                                    # nothing goes out before a wait or a full set
        res = [g.wait_handdec(t) for t in tk]
        n = len(members)
        assert 20 <= n <= 32 and g.handdec_stats() == (n, 1, n, 2)
        counts = [m.check(r) for m, r in zip(members, res)]
        assert len(set(counts)) > 4, counts
        assert any(c == m.case.params[2] for c, m in zip(counts, members)), counts  # at its max_hands
        assert any(c == 0 and m.rows for c, m in zip(counts, members)), counts      # rows, and no hand
        assert all(c == 0 for c, m in zip(counts, members) if not m.rows)
        assert len({m.case.params for m in members}) > 15 and any(m.case.params[3] is None for m in members)
    finally:
        _free(g, members)


@pytest.mark.parametrize("decoder", ["palm", "landmarks"])
def test_one_decoder_one_launch_and_a_set_without_rows(ctx, decoder):
    import mi355fx
    if decoder == "palm":
        members = [Member(ctx, M.palm_case(100 + k, N)) for k, N in enumerate((300, 1, 256, 77))]
    else:
        members = [Member(ctx, M.landmark_case(100 + k, Hn, D, kind)) for k, (Hn, D, kind) in enumerate(((9, 3, "full"), (1, 2, "absent"), (64, 2, "short"), (5, 16, "full")))]
    empty = [Member(ctx, M.palm_case(110, 0)), Member(ctx, M.landmark_case(111, 0, 3, "full")), Member(ctx, M.landmark_case(112, 0, 2, "absent"))]
    g = mi355fx.Group(0)
    try:
        _run_set(g, members)
        assert g.handdec_stats() == (4, 1, 4, 1)
        tk = [m.submit(g) for m in empty] + [g.submit_handdec_palm(ctx, None, 0, (0.5, 0.3, 2))]   # a null tensor is fine without rows
        assert len(set(tk)) == 4 and all(t > 0 for t in tk)
        for m, t in zip(empty + [empty[0]], tk):
            got = g.wait_handdec(t)
            assert len(got) == 0 if m.palm else (len(got[0]), len(got[1])) == (0, 0)
        assert g.handdec_stats() == (8, 2, 4, 1)                                    # no rows: no launch
        _run_set(g, [members[0], empty[0], empty[1], members[1]], reverse=True)     # ... and members without rows among others
        assert g.handdec_stats() == (12, 3, 4, 2)
    finally:
        _free(g, members + empty)


def test_submit_order_does_not_matter(ctx):
    import mi355fx
    members = [Member(ctx, c) for c in M.mixed_cases()[:12]]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members]
        fwd = [g.wait_handdec(t) for t in tk]
        tk = {k: members[k].submit(g) for k in reversed(range(len(members)))}
        rev = {k: g.wait_handdec(tk[k]) for k in reversed(range(len(members)))}
        assert g.handdec_stats() == (24, 2, 12, 4)
        for k, m in enumerate(members):
            m.check(fwd[k])
            a, b = (fwd[k], rev[k]) if m.palm else (fwd[k][0].tobytes() + fwd[k][1].tobytes(), rev[k][0].tobytes() + rev[k][1].tobytes())
            assert (a.tobytes() == b.tobytes()) if m.palm else a == b, m.case.name
    finally:
        _free(g, members)


def test_two_sets_and_the_first_sets_results_survive(ctx):
    """40 submits: sets of 32 and 8. The first set's tickets are collected only after the second set has been launched and collected."""
    import mi355fx
    members = [Member(ctx, M.palm_case(300 + k, (64, 257, 1, 2016)[(k // 2) % 4]) if k % 2 == 0 else M.landmark_case(300 + k, (3, 11, 1, 64)[(k // 2) % 4], (2, 3, 16)[k % 3],
                                                                                                                      ("absent", "short", "full")[(k // 2) % 3]))
               for k in range(40)]
    g = mi355fx.Group(0)
    try:
        lone = {m: m.lone() for m in members}
        tk = [m.submit(g) for m in members[:32]]
        assert g.handdec_stats() == (32, 1, 32, 2)                                  # the 32nd submit filled a set
        tk += [m.submit(g) for m in members[32:]]
        assert g.handdec_stats() == (32, 1, 32, 2)
        second = [m.check(g.wait_handdec(t), lone[m]) for m, t in zip(members[32:], tk[32:])]
        assert g.handdec_stats() == (40, 2, 32, 4)
        first = [m.check(g.wait_handdec(tk[k]), lone[members[k]]) for k, m in reversed(list(enumerate(members[:32])))]
        assert sum(first) > 40 and sum(second) > 8
        assert g.handdec_stats() == (40, 2, 32, 4)
    finally:
        _free(g, members)


def test_slots_stay_clean_over_intervals(ctx):
    """The same job slots over four intervals with different tensors in them: 4096 rows then 1 row, H = 64 then H = 1, many hands then
    none. Nothing on the device is cleared between sets, so a stale count or record of the earlier interval would show; and the caller's
    arrays keep their bytes from n_hands on."""
    import mi355fx
    many = M.palm_case(400, 4096, (0.1, 0.0, 8, (640, 360)))
    none = M.palm_case(401, 2016, (5.0, 0.3, 8, None))
    one = M.palm_case(402, 1, (-1.0, 0.0, 8, (192, 192)))
    h64 = M.landmark_case(403, 64, 3, "absent", (0.5, 0.0, 10, (640, 360)))
    h1 = M.landmark_case(404, 1, 3, "absent", (0.5, 0.2, 10, (640, 360)))
    h_none = M.landmark_case(405, 64, 2, "full", (5.0, 0.2, 10, None))
    cases = [many, none, one, h64, h1, h_none]
    mem = {c: Member(ctx, c) for c in cases}
    intervals = [[many, h64, many, h64], [one, h1, none, h_none], [none, h_none, one, h1], [many, h64, many, h64]]
    g = mi355fx.Group(0)
    try:
        lone = {c: mem[c].lone() for c in cases}
        assert len(lone[many]) == 8 and len(lone[none]) == 0 and len(lone[one]) == 1
        assert len(lone[h64][0]) >= 5 and len(lone[h1][0]) == 1 and len(lone[h_none][0]) == 0
        for interval in intervals:
            tk = [mem[c].submit(g) for c in interval]
            for c, t in zip(interval, tk):
                rc, dets, kps, n = _raw_wait(g, t)
                m = mem[c]
                assert rc == 0
                m.check(dets[:n].copy() if m.palm else (dets[:n].copy(), kps[:n].copy()), lone[c])
                assert (dets[n:].view(np.uint8) == FILL).all(), c.name              # records from n_hands on are not touched
                assert (kps[n if not m.palm else 0:].view(np.uint8) == FILL).all(), c.name
        assert g.handdec_stats() == (16, 4, 4, 8)
    finally:
        _free(g, list(mem.values()))


def _status(fn, *args):
    import mi355fx
    with pytest.raises(mi355fx.Mi355Error) as e:
        fn(*args)
    return e.value.status


def test_refusals_and_ticket_classes(ctx):
    import mi355fx
    INV, UNS = mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED
    pm, lm = Member(ctx, M.palm_case(500, 300)), Member(ctx, M.landmark_case(501, 6, 3, "full"))
    pic = np.random.default_rng(3).integers(0, 256, 64 * 48 * 4, dtype=np.uint8)
    d_pic, d_out = ctx.alloc(pic.nbytes), ctx.alloc(pic.nbytes)
    ctx.h2d(d_pic, pic)
    d_yolo = _upload(ctx, np.zeros(6 * 10, np.float32))
    g = mi355fx.Group(0)
    check = g.L.mi355_selftest_handdec_check
    P = (0.5, 0.3, 2, 0, 0)
    try:
        # (decoder, rows, D, num_scores, params): refused with the status the lone entry points' checks give
        shapes = [(0, 4097, 0, 0, P, UNS), (0, 300, 0, 0, (0.5, 0.3, 9, 0, 0), INV), (0, 300, 0, 0, (0.5, 0.3, 0, 0, 0), INV), (0, 300, 0, 0, (0.5, 0.3, 2, 192, 0), INV),
                  (0, 300, 0, 0, (0.5, 0.3, 2, -1, -1), INV), (1, 1025, 3, 0, P, UNS), (1, 6, 1, 0, P, INV), (1, 6, 17, 0, P, UNS), (1, 6, 3, 1025, P, UNS),
                  (1, 6, 3, 0, (0.5, 0.3, 11, 0, 0), INV), (1, 0, 1, 0, P, INV), (0, 0, 0, 0, (0.5, 0.3, 9, 0, 0), INV)]
        for decoder, rows, D, ns, p, status in shapes:
            row_bytes = 32 if decoder == 0 else 21 * D * 4
            assert check(decoder, rows * row_bytes, 1, rows, D, ns * 4, ns, p[2], p[3], p[4]) == status, (decoder, rows, D, ns, p)
            if decoder == 0:
                assert _status(g.submit_handdec_palm, ctx, pm.d, rows, p) == status, (rows, p)
            else:
                assert _status(g.submit_handdec_landmarks, ctx, lm.d, rows, D, p, lm.ds if ns else None, ns) == status, (rows, D, ns, p)
        assert check(1, 6 * 63 * 4, 1, 6, 3, 0, 1025, 2, 0, 0) == UNS               # ... and without a scores pointer num_scores is ignored
        t_ignored = g.submit_handdec_landmarks(ctx, lm.d, 6, 3, P, None, 1025)
        for call in (lambda: g.submit_handdec_palm(ctx, pm.d, 300, None), lambda: g.submit_handdec_palm(None, pm.d, 300, P), lambda: g.submit_handdec_palm(ctx, None, 300, P),
                     lambda: g.submit_handdec_palm(ctx, pm.d + 2, 300, P), lambda: g.submit_handdec_landmarks(ctx, None, 6, 3, P), lambda: g.submit_handdec_landmarks(ctx, lm.d + 1, 6, 3, P),
                     lambda: g.submit_handdec_landmarks(ctx, lm.d, 6, 3, P, lm.ds + 2, 6), lambda: g.submit_handdec_landmarks(ctx, lm.d, 6, 3, None),
                     lambda: g.wait_handdec(0), lambda: g.wait_handdec(12345)):
            assert _status(call) == INV
        hp = mi355fx.HandParams(0.5, 0.3, 2, 0, 0)
        assert g.L.mi355_group_submit_handdec_palm(g.h, ctx.h, pm.d, 300, C.byref(hp), None) == INV                      # null ticket
        assert g.L.mi355_group_submit_handdec_landmarks(g.h, ctx.h, lm.d, 6, 3, None, 0, C.byref(hp), None) == INV
        assert g.L.mi355_group_submit_handdec_palm(None, ctx.h, pm.d, 300, C.byref(hp), C.byref(C.c_uint64(0))) == INV   # null group
        assert g.handdec_stats() == (0, 0, 0, 0)
        g.wait_all()
        assert g.handdec_stats() == (1, 1, 1, 1)                                    # the refused submits queued nothing: the one accepted tensor
        a = lm.own.handdec_landmarks_device(lm.d, 6 * 63 * 4, 1, 6, 3, [P])[0]
        b = g.wait_handdec(t_ignored)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        tp, tl = pm.submit(g), lm.submit(g)
        # a null kps on a landmark ticket is refused and the ticket is then collected; a palm ticket ignores kps
        rc, _, _, n = _raw_wait(g, tl, null_kps=True)
        assert rc == INV and n == 77
        assert g.L.mi355_group_wait_handdec(g.h, tl, None, None, None) == INV
        # tickets of the other queues are refused here and stay collectable there
        t_pair = g.submit_compare(ctx, d_pic, d_pic, 256, 64, 48, "RGBA", 5)
        t_cd = g.submit_colordetect(ctx, d_pic, pic.nbytes, "RGBA", 10, 2)
        t_hd = g.submit_hsvdetect(ctx, d_pic, 256, "RGBx", d_out, 256, "RGBA", 64, 48, (120.0, 40.0, 0.8, 0.5, 0.7, 0.6))
        t_yd = g.submit_yolodec(ctx, d_yolo, "X", 6, 10, (0.5, 0.5, 0.5))
        for other in (t_pair, t_cd, t_hd, t_yd):
            assert _status(g.wait_handdec, other) == INV
        # ... and the reverse
        for refuse in (g.wait, lambda tt: g.order_after(ctx, tt), g.wait_compare, g.wait_colordetect, g.wait_hsvdetect, g.wait_yolodec):
            for t in (tp, tl):
                assert _status(refuse, t) == INV
        assert g.handdec_stats() == (1, 1, 1, 1)
        assert g.wait_compare(t_pair)[0] == 0.0
        assert 1 <= len(g.wait_colordetect(t_cd)) <= 2
        g.wait_hsvdetect(t_hd)
        assert g.wait_yolodec(t_yd)[1] == 0
        assert g.handdec_stats() == (1, 1, 1, 1)                                    # the other queues' launches are theirs
        lm.check(g.wait_handdec(tl))                                                # collectable after its refusals
        rc, dets, _, n = _raw_wait(g, tp, null_kps=True)                            # a palm ticket needs no kps
        assert rc == 0
        pm.check(dets[:n].copy())
        assert g.handdec_stats() == (3, 2, 2, 3)
        for t in (tp, tl):
            assert _status(g.wait_handdec, t) == INV                                # collected once
        assert g.handdec_stats() == (3, 2, 2, 3)
    finally:
        _free(g, [pm, lm])
        for p in (d_pic, d_out, d_yolo):
            ctx.free(p)


@pytest.mark.parametrize("what", ["palm_tensor", "landmark_scores"])
def test_a_tensor_is_read_after_what_its_stream_held(ctx, what):
    """The tensor (the scores vector) is written by a device copy on the member's stream immediately before the submit, behind four
    64 MiB copies that keep the stream busy, with no synchronisation: the set, on the queue's own stream, must wait for it."""
    import mi355fx
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3
    if what == "palm_tensor":
        p = (0.3, 0.1, 8, (640, 360))
        real, decoy = M.palm_case(600, 1000, p), M.palm_case(601, 1000, p)
        new = real.data
    else:
        p = (0.5, 0.1, 10, (640, 360))
        real = M.landmark_case(602, 40, 3, "full", p)
        decoy = H.LandmarkCase("decoy", real.data, np.random.default_rng(77).uniform(0, 1, len(real.scores)).astype(np.float32), p)
        new = real.scores
    m = Member(ctx, decoy)                                                          # the device holds the decoy for now
    stage = ctx.alloc(new.nbytes)
    ctx.h2d(stage, new)
    filler = 64 << 20
    a, b = ctx.alloc(filler), ctx.alloc(filler)
    g = mi355fx.Group(0)
    try:
        old = m.lone()
        m.check(old, old)
        for _ in range(4):
            assert hip.hipMemcpyAsync(b, a, filler, D2D, ctx.stream) == 0
        assert hip.hipMemcpyAsync(m.d if m.palm else m.ds, stage, new.nbytes, D2D, ctx.stream) == 0
        t = m.submit(g)
        got = g.wait_handdec(t)
        m.case = real                                                               # what the device holds now
        m.check(got)
        assert (got.tobytes() != old.tobytes()) if m.palm else (got[0].tobytes() != old[0].tobytes())
    finally:
        _free(g, [m])
        for q in (stage, a, b):
            ctx.free(q)


def test_rendezvous_threads(mi355lib):
    """Eight instances on eight threads x 20 intervals, each with its own context - four palm and four landmark members - submitting
    and waiting at once (what transform_ip does); rendezvous 8 with a 2 ms linger. One thread sits out every third interval."""
    import mi355fx
    n, rounds = 8, 20
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    cases = [M.palm_case(700 + s, (300, 2016, 1, 1025)[s // 2]) if s % 2 == 0 else M.landmark_case(700 + s, (2, 11, 64, 5)[s // 2], (3, 2, 16, 3)[s // 2],
                                                                                                   ("full", "absent", "short", "full")[s // 2]) for s in range(n)]
    members = [Member(ctxs[0], case, ctx=c) for case, c in zip(cases, ctxs)]
    g = mi355fx.Group(0)
    g.set_handdec_rendezvous(n, 2000)
    try:
        lone = [m.lone() for m in members]
        for m, l in zip(members, lone):
            m.check(l, l)                                                           # the lone answers against the restatement, once
        as_bytes = lambda m, r: r.tobytes() if m.palm else r[0].tobytes() + r[1].tobytes()
        bar = threading.Barrier(n)
        errors, seen = [], [0] * n

        def element(s):
            try:
                for r in range(rounds):
                    bar.wait()
                    if s == 5 and r % 3 == 2:
                        continue
                    got = g.wait_handdec(members[s].submit(g))
                    assert as_bytes(members[s], got) == as_bytes(members[s], lone[s]), (s, r)
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
        st = g.handdec_stats()
        assert sum(seen) == total == st[0] and st[2] <= n and rounds <= st[1] <= total and st[3] <= 2 * st[1]
    finally:
        _free(g, members)
        for c in ctxs:
            c.close()


def test_flush_wait_all_and_destroy_cover_the_queue(ctx):
    import mi355fx
    members = [Member(ctx, M.palm_case(800 + k, 200 + 57 * k) if k % 2 == 0 else M.landmark_case(800 + k, 4 + k, 3, "full")) for k in range(4)]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members[:2]]
        g.flush()
        assert g.handdec_stats() == (2, 1, 2, 2)                                    # flush launches the queue
        tk += [m.submit(g) for m in members[2:]]
        g.wait_all()                                                                # launches and waits; results stay collectable
        assert g.handdec_stats() == (4, 2, 2, 4)
        for m, t in zip(members, tk):
            m.check(g.wait_handdec(t))
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


def _hand_with_box(bbox, wrist_to_base=(0.0, -1.0), D=2):
    """One hand whose PADDED box (0.15 of the width and height on each side) is bbox, to f32 rounding; the vector from the wrist (point
    0) to the middle-finger base (point 9) has the given direction: (0, -1) is rotation 0."""
    x0, y0, x1, y1 = bbox
    w, h = (x1 - x0) / 1.3, (y1 - y0) / 1.3
    mnx, mny = x0 + 0.15 * w, y0 + 0.15 * h
    pts = np.zeros((21, D), np.float64)
    pts[:, 0], pts[:, 1] = mnx + w / 2, mny + h / 2
    pts[1, :2], pts[2, :2] = (mnx, mny), (mnx + w, mny + h)
    pts[0, :2] = (mnx + w / 2, mny + h / 2)
    pts[9, :2] = (mnx + w / 2 + wrist_to_base[0] * w / 4, mny + h / 2 + wrist_to_base[1] * h / 4)
    return pts.reshape(1, -1).astype(np.float32)


def test_the_committed_known_answers_share_one_set(ctx):
    """tests/golden/handdec_reference_kats.json (the numbers of the reference's own unit tests) as members of one set. The box cases
    are landmark hands whose padded box is the case's box: floor / ceil leave f32 rounding of the construction no say. The degenerate
    box cannot come out of either decoder - a hand without width is dropped before the oriented-box rule - so it must yield no hand.
    The palm rotation case keeps the direction of its keypoint vector at a length a valid palm can have."""
    import mi355fx
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "handdec_reference_kats.json")))
    boxes = golden["oriented_od_params"] + [dict(golden["rotation_mapping"], name="rotation_mapping")]
    cases, wants = [], []
    for k in boxes:
        cases.append(H.LandmarkCase(k["name"], _hand_with_box(k["bbox"]), None, (0.5, 0.2, 10, tuple(k["frame"]))))
        wants.append(("box", k))
    for k in golden["rotation_checks"]:
        if k["name"] == "angle_from_vector":
            cases.append(H.LandmarkCase("angle_%s_%s" % (k["dx"], k["dy"]), _hand_with_box([10, 10, 50, 50], (k["dx"], k["dy"])), None, (0.5, 0.2, 10, (100, 100))))
        elif k["name"] == "palm_rotation_from_keypoints":
            d = (np.float64(k["kp2"]) - np.float64(k["kp0"])) * 0.1
            cases.append(H.PalmCase(k["name"], [(0.9, 0.5, 0.5, 0.2, 0.5, 0.5, 0.5 + d[0], 0.5 + d[1])], (0.5, 0.3, 2, None)))
        else:
            pts = np.zeros((1, 21, k["kps_dim"]), np.float32)
            pts[0, 0, :2], pts[0, 9, :2] = k["wrist"], k["middle_base"]
            pts[0, 5, :2] = (3.0, 4.0)                                              # a box: the all-zero hand of the reference's test has none
            cases.append(H.LandmarkCase(k["name"], pts.reshape(1, -1), None, (0.5, 0.2, 2, (100, 100))))
        wants.append(("rotation", k))
    members = [Member(ctx, c) for c in cases]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members]
        res = [g.wait_handdec(t) for t in reversed(tk)][::-1]
        assert g.handdec_stats() == (len(members), 1, len(members), 2)
        for m, r, (kind, k) in zip(members, res, wants):
            m.check(r)
            dets = r if m.palm else r[0]
            if kind == "box" and k["name"] == "drop_degenerate_box":
                assert len(dets) == 0
            elif kind == "box" and k["name"] == "rotation_mapping":
                assert len(dets) == 1 and dets["has_od"][0] == 1 and dets["rotation"][0] == 0
                assert abs(float(dets["rotation_od"][0]) + np.pi / 2) < k["expect_rotation_od_plus_frac_pi_2_abs_below"]
            elif kind == "box":
                assert len(dets) == 1, k["name"]
                d = dets[0]
                got = [int(d["x"]), int(d["y"]), int(d["width"]), int(d["height"])] if d["has_od"] else None
                assert got == k["expect"], (k["name"], got)
                assert d["rotation"] == 0 and (not d["has_od"] or abs(float(d["rotation_od"]) + np.pi / 2) < 1e-6), k["name"]
            elif k["name"] == "landmark_rotation_aligns_with_hand_axis":
                assert len(dets) == 1 and dets["has_od"][0] == 1 and abs(float(dets["rotation_od"][0]) - k["expect_rotation_od"]) < k["abs_below"]
            elif k["name"] == "palm_rotation_from_keypoints":
                assert len(dets) == 1 and abs(float(dets["rotation"][0]) - k["expect"]) < k["abs_below"]
            else:
                assert len(dets) == 1 and abs(float(dets["rotation"][0]) - np.pi / 2 - k["expect"]) < k["abs_below"], k
    finally:
        _free(g, members)
