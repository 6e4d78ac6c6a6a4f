"""GPU tests for yoloxinference frames in the decoder queue of the dispatcher (mi355_group_submit_yolox_infer, collected with
mi355_group_wait_yolodec): RGB frames of INDEPENDENT `yoloxinference ! yoloxtensordec` pipelines that share one
finalized net, as members of the launch sets the decoded tensors and the head maps use - one conversion launch
(yolox_input_jobs_kernel), ONE forward per (net, frame size) in an activation lane of the queue's own, then the head score / NMS job
launches and the set's one download.

The bar for every member, three ways: the full count; got.tobytes() equal to the lone one-frame mi355_yolox_infer_dets_device on the
same net and frame; and the bars tests/test_gpu_yolox_net.py::test_compositions_bit_for_bit holds that lone call to - with the case's
own thresholds, which stand in the widest gap of the f64 maps, between one detection and the f64 survivors, at most A / 2.

Nets and frames come from tests/yolox_net_cases.py: nano (the depthwise path) with 3 classes and tiny with 1, at 64 x 96 and at 32 x 32
(a 1 x 1 top level). One net serves both sizes (that is the point of test 4), so its prediction layers are the ones rescaled at
64 x 96 and the thresholds of its 32 x 32 frames are chosen from the f64 maps of those frames under the same parameters."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import test_gpu_group_yolox_head as GH
import yolox_head_cases as HC
import yolox_net_cases as K

pytestmark = pytest.mark.gpu

FILL = 201                      # the bytes around a frame's pixels: row padding, the bytes in front of a shifted base pointer


class SharedNetCase(K.CompositionCase):
    """Frames of another size through the net of `base`: its parameters, thresholds from these frames' own f64 maps."""

    def __init__(self, base, H, W, n_frames=3):
        self._base = base
        super().__init__(base.config, base.C, H, W, n_frames)

    @property
    def P(self):
        return self._base.P


@functools.lru_cache(maxsize=None)
def case_of(config, num_classes, H=64, W=96):
    base = K.CompositionCase(config, num_classes, 64, 96, 3)
    return base if (H, W) == (64, 96) else SharedNetCase(base, H, W)


def device_net(ctx, case):
    import mi355fx
    net = mi355fx.YoloxNet(ctx, case.cfg())
    net.load(case.P)
    net.finalize()
    return net


class FrameMember:
    """One instance's RGB frame in a device buffer of its own - `pad` bytes of row padding, the base pointer `off` bytes into the
    allocation - with its settings and its output capacity; c: the context that owns the buffer, ctx: the member's stream."""

    def __init__(self, c, net, case, f, pad=0, off=0, params=None, max_dets=None, ctx=None):
        self.c, self.own, self.net, self.case, self.f = c, ctx or c, net, case, f
        self.H, self.W, self.A = case.H, case.W, case.A
        self.stock = params is None
        self.params = tuple(float(np.float32(v)) for v in (case.params if params is None else params))
        self.cap = self.A if max_dets is None else max_dets
        self.stride = 3 * self.W + pad
        self.host = self.image(case.frames[f], off)
        self.d = c.alloc(self.host.nbytes)
        c.h2d(self.d, self.host)
        self.ptr = self.d + off
        self.name = "%s-f%d-pad%d-off%d" % (case.name, f, pad, off)

    def image(self, frame, off):
        buf = np.full(off + self.H * self.stride, FILL, np.uint8)
        buf[off:].reshape(self.H, self.stride)[:, :3 * self.W] = frame.reshape(self.H, 3 * self.W)
        return buf

    def submit(self, g):
        return g.submit_yolox_infer(self.own, self.net, self.ptr, self.stride, self.W, self.H, self.params, self.cap)

    def lone(self):
        got, n = self.net.infer_dets_device(self.ptr, 0, self.stride, 1, self.W, self.H, [self.params], self.cap, return_counts=True)
        return got[0], n[0]

    def check(self, result, lone=None):
        got, n = result
        lone_got, lone_n = lone or self.lone()
        assert n == lone_n, (self.name, n, lone_n)                                  # the full count, even above the capacity
        assert len(got) == min(n, self.cap), (self.name, len(got), n, self.cap)
        assert got.tobytes() == lone_got.tobytes(), self.name
        if self.stock:                                                              # the bars of test_compositions_bit_for_bit
            assert 1 <= n <= self.case.survivors[self.f] <= self.A // 2, (self.name, n, self.case.survivors[self.f])
        return n

    def free(self):
        self.c.free(self.d)


def _close(g, members, nets):
    if g is not None:
        g.close()
    for m in members:
        m.free()
    for net in nets:
        net.close()


# (pad, off): packed rows; padded rows, which leave most rows off a 4-byte boundary; a base pointer off by one byte
LAYOUTS = ((0, 0), (5, 0), (0, 1))


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("config,num_classes,H,W", [("nano", 3, 64, 96), ("tiny", 1, 32, 32)])
def test_one_class(ctx, config, num_classes, H, W, n):
    """1: n members of one class, each with a buffer of its own: one upload, the conversion launch, ONE forward of n frames, the two head
    launches, one set (so one download)."""
    import mi355fx
    case = case_of(config, num_classes, H, W)
    net = device_net(ctx, case)
    members = [FrameMember(ctx, net, case, f, *LAYOUTS[f]) for f in range(n)]
    g = mi355fx.Group(0)
    try:
        L = net.launches()
        tk = [m.submit(g) for m in members]
        assert g.yolodec_stats() == (0, 0, 0, 0) and g.yolox_infer_stats() == (0, 0, 0, 0, 0, 0)   # nothing goes out before a wait
        res = [g.wait_yolodec(t) for t in tk]
        assert g.yolodec_stats() == (n, 1, n, 1 + L + 2)                            # a member counts as a tensor, its launches among the set's
        assert g.yolox_head_stats() == (n, 1, 1, 2)                                 # ... and as a head from the score launch on; one upload
        assert g.yolox_infer_stats() == (n, 1, n, 1 + L, 1, 2)                      # one forward of n frames; a lane: its input tensor and its arena
        counts = [m.check(r) for m, r in zip(members, res)]
        assert all(c >= 1 for c in counts)
        # the same members again: the lane is reused, counters and keys are clean
        res = [g.wait_yolodec(t) for t in [m.submit(g) for m in members]]
        for m, r in zip(members, res):
            m.check(r)
        assert g.yolox_infer_stats() == (2 * n, 2, n, 2 * (1 + L), 1, 2)
    finally:
        _close(g, members, [net])


def test_own_settings_and_capacities(ctx):
    """2: every member its own thresholds and its own capacity: none at all, one below the count, a few, more than A."""
    import mi355fx
    case = case_of("nano", 3)
    net = device_net(ctx, case)
    g = mi355fx.Group(0)
    members = []
    try:
        probe = FrameMember(ctx, net, case, 0)
        members.append(probe)
        full = probe.lone()[1]
        box, cls, _ = case.params
        members += [FrameMember(ctx, net, case, 0, max_dets=0),
                    FrameMember(ctx, net, case, 0, max_dets=max(full - 1, 0)),
                    FrameMember(ctx, net, case, 1, pad=5, max_dets=case.A + 7),
                    FrameMember(ctx, net, case, 1, params=(box, cls, 0.05), max_dets=3),
                    FrameMember(ctx, net, case, 2, off=1, params=(0.0, 0.0, 0.9)),       # every candidate survives the thresholds
                    FrameMember(ctx, net, case, 2, params=(2.0, 0.0, 0.5))]              # none does: no sigmoid reaches 2
        tk = [m.submit(g) for m in members]
        res = [g.wait_yolodec(t) for t in tk]
        counts = [m.check(r) for m, r in zip(members, res)]
        assert g.yolox_infer_stats()[:3] == (len(members), 1, len(members))
        assert counts[1] == counts[2] == full >= 1 and len(res[1][0]) == 0 and len(res[2][0]) == full - 1
        assert len(res[3][0]) == counts[3] and counts[6] == 0 and counts[5] >= 1
        assert res[2][0].tobytes() == res[0][0][:full - 1].tobytes()                # a smaller capacity truncates, nothing else
    finally:
        _close(g, members, [net])


def _mixed_set(ctx, nets, order):
    """two nets, a submitted head, an X tensor and a V8 tensor in ONE set, submitted in `order`; returns what each member got"""
    import mi355fx
    nano, tiny = case_of("nano", 3), case_of("tiny", 1)
    members = [FrameMember(ctx, nets[0], nano, 0, pad=5),
               GH.TensorMember(ctx, GH._tensor(1, "V8", 84, 300)),
               FrameMember(ctx, nets[1], tiny, 1, off=1),
               GH.HeadMember(ctx, HC.shape_head("boundary255", 80), "one", params=(0.45, 0.4, 0.3)),
               FrameMember(ctx, nets[0], nano, 2, max_dets=2),
               GH.TensorMember(ctx, GH._tensor(2, "X", 9, 257))]
    g = mi355fx.Group(0)
    try:
        tk = {k: members[k].submit(g) for k in order}
        assert g.yolodec_stats() == (0, 0, 0, 0)
        res = {k: g.wait_yolodec(tk[k]) for k in order}
        # the conversion, a forward per net, the V8 and X score launches, the tensors' NMS, the heads' score and NMS
        launches = 1 + nets[0].launches() + nets[1].launches()
        assert g.yolodec_stats() == (6, 1, 6, launches + 5)
        assert g.yolox_head_stats() == (4, 1, 1, 2)                                 # three infer members and the submitted head: one table upload
        assert g.yolox_infer_stats() == (3, 2, 2, launches, 2, 4)
        for k, m in enumerate(members):
            m.check(res[k])
        return [(res[k][0].tobytes(), res[k][1]) for k in range(len(members))]
    finally:
        g.close()
        for m in members:
            m.free()


def test_a_mixed_set_in_both_orders(ctx):
    """3 and 5: every member against its lone form, the launch count against the formula; in reverse submit order - the classes are
    numbered the other way round, every member is another frame of its forward - each member's bytes are unchanged."""
    nets = [device_net(ctx, case_of("nano", 3)), device_net(ctx, case_of("tiny", 1))]
    try:
        forward = _mixed_set(ctx, nets, list(range(6)))
        backward = _mixed_set(ctx, nets, list(reversed(range(6))))
        assert forward == backward
    finally:
        for net in nets:
            net.close()


@pytest.mark.parametrize("reverse", [False, True])
def test_one_net_at_two_sizes_in_one_set(ctx, reverse):
    """4 (and 5): one net at 32 x 32 and at 64 x 96, interleaved in submit order. The head launches run after BOTH forwards: with one
    lane per net the second forward's level buffers would overwrite the first's."""
    import mi355fx
    big, small = case_of("nano", 3), case_of("nano", 3, 32, 32)
    net = device_net(ctx, big)
    members = [FrameMember(ctx, net, (small, big)[k % 2], k // 2, *LAYOUTS[k % 3]) for k in range(6)]
    g = mi355fx.Group(0)
    try:
        order = list(reversed(range(6))) if reverse else list(range(6))
        tk = {k: members[k].submit(g) for k in order}
        res = {k: g.wait_yolodec(tk[k]) for k in order}
        L = net.launches()
        assert g.yolodec_stats() == (6, 1, 6, 1 + 2 * L + 2)
        assert g.yolox_infer_stats() == (6, 2, 3, 1 + 2 * L, 2, 4)                  # two classes of three frames, a lane each
        for k, m in enumerate(members):
            m.check(res[k])
    finally:
        _close(g, members, [net])


def test_33_members_make_two_sets(ctx):
    """6: a full set goes out with the 32nd submit, the 33rd member waits for its own; the second set's ticket is collected first."""
    import mi355fx
    case = case_of("tiny", 1, 32, 32)
    net = device_net(ctx, case)
    members = [FrameMember(ctx, net, case, k % 3, *LAYOUTS[(k // 3) % 3]) for k in range(33)]
    g = mi355fx.Group(0)
    try:
        L = net.launches()
        tk = [m.submit(g) for m in members]
        assert g.yolodec_stats() == (32, 1, 32, 1 + L + 2)                          # submit launches a full set
        lone = {(m.f, m.stride, m.ptr - m.d): m.lone() for m in members[:9]}        # nine distinct (frame, layout) pairs
        last = g.wait_yolodec(tk[32])
        assert g.yolodec_stats() == (33, 2, 32, 2 * (1 + L + 2))
        members[32].check(last, lone[(members[32].f, members[32].stride, members[32].ptr - members[32].d)])
        for m, t in zip(members[:32], tk[:32]):
            m.check(g.wait_yolodec(t), lone[(m.f, m.stride, m.ptr - m.d)])
        assert g.yolox_infer_stats() == (33, 2, 32, 2 * (1 + L), 1, 2)              # frames in the largest forward: 32; the lane of 32 serves the set of one
    finally:
        _close(g, members, [net])


def test_the_frame_is_read_after_what_its_stream_held(ctx):
    """7: the frame is written by a device copy on the member's stream immediately before the submit, behind four 64 MiB copies that
    keep the stream busy, with no synchronisation: the set, on the queue's own stream, must wait for it."""
    import mi355fx
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3
    case = case_of("nano", 3)
    net = device_net(ctx, case)
    m, r = FrameMember(ctx, net, case, 0, pad=5), FrameMember(ctx, net, case, 1, pad=5)   # m's buffer holds the decoy frame for now
    filler = 64 << 20
    a, b = ctx.alloc(filler), ctx.alloc(filler)
    g = mi355fx.Group(0)
    try:
        old, want = m.lone(), r.lone()
        assert old[0].tobytes() != want[0].tobytes()
        for _ in range(4):
            assert hip.hipMemcpyAsync(b, a, filler, D2D, ctx.stream) == 0
        assert hip.hipMemcpyAsync(m.d, r.d, r.host.nbytes, D2D, ctx.stream) == 0
        got = g.wait_yolodec(m.submit(g))
        m.f = 1                                                                     # what the buffer holds now
        m.check(got, want)
    finally:
        _close(g, [m, r], [net])
        for p in (a, b):
            ctx.free(p)


def test_four_threads_share_one_net(mi355lib):
    """8: four instances on four threads, each with a context of its own, one net (owned by a fifth context), rendezvous of 4: every
    interval is one set with ONE forward of 4 frames."""
    import mi355fx
    n, rounds = 4, 3
    owner = mi355fx.Context(0)
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    case = case_of("nano", 3)
    net = device_net(owner, case)
    members = [FrameMember(owner, net, case, s % 3, *LAYOUTS[s % 3], ctx=c) for s, c in enumerate(ctxs)]
    g = mi355fx.Group(0)
    g.set_yolodec_rendezvous(n, 5000000)     # (nobody lingers: the fourth submit of an interval finds the set full and launches it)
    try:
        lone = [m.lone() for m in members]
        for m, l in zip(members, lone):
            m.check(l, l)
        bar = threading.Barrier(n)
        errors = []

        def element(s):
            try:
                for r in range(rounds):
                    bar.wait()
                    got, cnt = g.wait_yolodec(members[s].submit(g))
                    assert cnt == lone[s][1] and got.tobytes() == lone[s][0].tobytes(), (s, r)
            except Exception as e:                 # noqa: BLE001 - told to the main thread
                errors.append(e)
                bar.abort()

        ts = [threading.Thread(target=element, args=(s,)) for s in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        L = net.launches()
        assert g.yolodec_stats() == (n * rounds, rounds, n, rounds * (1 + L + 2))
        assert g.yolox_infer_stats() == (n * rounds, rounds, n, rounds * (1 + L), 1, 2)
    finally:
        _close(g, members, [net])
        for c in ctxs + [owner]:
            c.close()


def test_the_owner_goes_on_using_its_net(ctx):
    """9: a set in flight, then lone calls on the same net by its owner - another frame, a batch of three, at another size - then the
    wait: the queue runs in lanes of its own, so every result is right."""
    import mi355fx
    big, small = case_of("nano", 3), case_of("nano", 3, 32, 32)
    net = device_net(ctx, big)
    members = [FrameMember(ctx, net, big, f, *LAYOUTS[f]) for f in range(3)] + [FrameMember(ctx, net, small, 0)]
    g = mi355fx.Group(0)
    try:
        want = [m.lone() for m in members]
        arena = net.arena_info()
        tk = [m.submit(g) for m in members[:2]]
        g.flush()                                                                   # the set is on the queue's stream now
        between = [members[3].lone(), members[2].lone()]                            # the owner's own arena, planned for other shapes
        members[3].check(between[0], want[3])
        members[2].check(between[1], want[2])
        for m, t, w in zip(members, tk, want):
            m.check(g.wait_yolodec(t), w)
        assert net.arena_info() == arena                                            # the queue never touched the net's own lane
        # ... and the other way round: pending (not launched) while the owner works
        t = members[0].submit(g)
        members[1].check(members[1].lone(), want[1])
        members[0].check(g.wait_yolodec(t), want[0])
    finally:
        _close(g, members, [net])


def test_lanes_grow_once(ctx):
    """10: sets of 3, 1 and 3 members: the lane allocates with the first set and never again; a second size is a second lane."""
    import mi355fx
    big, small = case_of("tiny", 1), case_of("tiny", 1, 32, 32)
    net = device_net(ctx, big)
    members = [FrameMember(ctx, net, big, f, *LAYOUTS[f]) for f in range(3)] + [FrameMember(ctx, net, small, f) for f in range(2)]
    g = mi355fx.Group(0)
    try:
        want = [m.lone() for m in members]
        L = net.launches()
        for k, take in enumerate(([0, 1, 2], [2], [1, 0, 2])):
            tk = [members[j].submit(g) for j in take]
            for j, t in zip(take, tk):
                members[j].check(g.wait_yolodec(t), want[j])
            assert g.yolox_infer_stats()[4:] == (1, 2), k                           # lanes alive, device allocations made for lanes
        assert g.yolox_infer_stats() == (7, 3, 3, 3 * (1 + L), 1, 2)
        for take in ([3, 4], [4], [0, 3]):
            tk = [members[j].submit(g) for j in take]
            for j, t in zip(take, tk):
                members[j].check(g.wait_yolodec(t), want[j])
            assert g.yolox_infer_stats()[4:] == (2, 4)
        assert g.yolox_infer_stats()[:3] == (12, 7, 3)
    finally:
        _close(g, members, [net])


def test_release_yolox_net(ctx):
    """11: refused while a ticket is uncollected (pending, in flight or finished), and the ticket stays collectable; after collection
    the lanes go; a new net of another config (perhaps at the old one's address) never meets a stale lane."""
    import mi355fx
    INV = mi355fx.ERR_INVALID_ARG
    first, second = case_of("nano", 3), case_of("tiny", 1)
    net = device_net(ctx, first)
    other = device_net(ctx, second)
    members = [FrameMember(ctx, net, first, 0), FrameMember(ctx, net, case_of("nano", 3, 32, 32), 1), FrameMember(ctx, other, second, 2)]
    g = mi355fx.Group(0)
    try:
        g.release_yolox_net(net)                                                    # a queue that has never run: nothing to free
        want = [m.lone() for m in members]
        tk = [m.submit(g) for m in members]
        for stage in ("pending", "in flight", "finished"):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.release_yolox_net(net)
            assert e.value.status == INV, stage
            if stage == "pending":
                g.flush()
            elif stage == "in flight":
                g.wait_all()
        assert g.yolox_infer_stats()[4:] == (3, 6)
        members[0].check(g.wait_yolodec(tk[0]), want[0])
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.release_yolox_net(net)                                                # one of its two tickets is still to be collected
        assert e.value.status == INV
        members[1].check(g.wait_yolodec(tk[1]), want[1])
        g.release_yolox_net(net)                                                    # the other net's ticket does not hold this one
        assert g.yolox_infer_stats()[4:] == (1, 6)
        g.release_yolox_net(net)                                                    # again: nothing left, no error
        members[2].check(g.wait_yolodec(tk[2]), want[2])
        # the net goes, one of the other config comes
        members[0].free(), members[1].free()
        net.close()
        net = device_net(ctx, second)
        members[0], members[1] = FrameMember(ctx, net, second, 0, pad=5), FrameMember(ctx, net, second, 1, off=1)
        tk = [m.submit(g) for m in members]
        for m, t in zip(members, tk):
            m.check(g.wait_yolodec(t))
        assert g.yolox_infer_stats()[4:] == (2, 8)                                  # the new net's lane beside the other's
        g.release_yolox_net(other)
        g.release_yolox_net(net)
        assert g.yolox_infer_stats()[4:] == (0, 8)
        assert g.L.mi355_group_release_yolox_net(g.h, None) == INV and g.L.mi355_group_release_yolox_net(None, net.h) == INV
    finally:
        _close(g, members, [net, other])


def test_refusals_and_ticket_classes(ctx):
    """12: a refused submit has the lone call's status and queues nothing; an infer ticket is a decoder ticket."""
    import mi355fx
    INV, UNS, NOT = mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED, mi355fx.ERR_NOT_CONFIGURED
    case = case_of("nano", 3)
    net = device_net(ctx, case)
    raw = mi355fx.YoloxNet(ctx, case.cfg())                                         # never finalized
    m = FrameMember(ctx, net, case, 0)
    pic = np.random.default_rng(3).integers(0, 256, 64 * 48 * 4, dtype=np.uint8)
    d_pic = ctx.alloc(pic.nbytes)
    ctx.h2d(d_pic, pic)
    g = mi355fx.Group(0)
    P = case.params
    try:
        cases = [
            (lambda: g.submit_yolox_infer(ctx, raw, m.ptr, m.stride, 96, 64, P, 10), NOT),       # before finalize
            (lambda: g.submit_yolox_infer(ctx, net, m.ptr, m.stride, 96, 48, P, 10), INV),       # H no multiple of 32
            (lambda: g.submit_yolox_infer(ctx, net, m.ptr, m.stride, 33, 64, P, 10), INV),
            (lambda: g.submit_yolox_infer(ctx, net, m.ptr, m.stride, 0, 64, P, 10), INV),
            (lambda: g.submit_yolox_infer(ctx, net, m.ptr, 3 * 2080, 2080, 32, P, 10), UNS),     # a side above 2048
            (lambda: g.submit_yolox_infer(ctx, net, m.ptr, 3 * 96 - 1, 96, 64, P, 10), INV),     # stride below the row
            (lambda: g.submit_yolox_infer(ctx, net, None, m.stride, 96, 64, P, 10), INV),        # null frame
            (lambda: g.submit_yolox_infer(None, net, m.ptr, m.stride, 96, 64, P, 10), INV),      # null context
            (lambda: g.submit_yolox_infer(ctx, None, m.ptr, m.stride, 96, 64, P, 10), INV),      # null net
            (lambda: g.submit_yolox_infer(ctx, net, m.ptr, m.stride, 96, 64, None, 10), INV),    # null settings
        ]
        for call, status in cases:
            with pytest.raises(mi355fx.Mi355Error) as e:
                call()
            assert e.value.status == status
        # the lone call gives one frame the same status
        for (w, h, stride, frame, which), status in (((96, 48, m.stride, m.ptr, net), INV), ((2080, 32, 3 * 2080, m.ptr, net), UNS), ((96, 64, 3 * 96 - 1, m.ptr, net), INV),
                                                     ((96, 64, m.stride, None, net), INV), ((96, 64, m.stride, m.ptr, raw), NOT)):
            with pytest.raises(mi355fx.Mi355Error) as e:
                which.infer_dets_device(frame, 0, stride, 1, w, h, [P], 10)
            assert e.value.status == status
        p, t64 = C.byref(mi355fx.YoloParams(*P)), C.c_uint64(0)
        assert g.L.mi355_group_submit_yolox_infer(g.h, ctx.h, net.h, m.ptr, m.stride, 96, 64, p, 10, None) == INV            # null ticket
        assert g.L.mi355_group_submit_yolox_infer(None, ctx.h, net.h, m.ptr, m.stride, 96, 64, p, 10, C.byref(t64)) == INV   # null group
        assert g.L.mi355_group_yolox_infer_stats(g.h, None) == INV and g.L.mi355_group_yolox_infer_stats(None, (C.c_uint64 * 6)()) == INV
        g.flush()
        assert g.yolodec_stats() == (0, 0, 0, 0) and g.yolox_head_stats() == (0, 0, 0, 0) and g.yolox_infer_stats() == (0, 0, 0, 0, 0, 0)
        t = m.submit(g)
        # tickets of the other queues are refused by the decoder queue's wait; an infer ticket is refused by theirs and stays collectable
        t_pair = g.submit_compare(ctx, d_pic, d_pic, 256, 64, 48, "RGBA", 5)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_yolodec(t_pair)
        assert e.value.status == INV
        for refuse in (g.wait, lambda tt: g.order_after(ctx, tt), g.wait_compare, g.wait_colordetect, g.wait_hsvdetect, g.wait_handdec):
            with pytest.raises(mi355fx.Mi355Error) as e:
                refuse(t)
            assert e.value.status == INV
        assert g.yolodec_stats() == (0, 0, 0, 0)
        assert g.wait_compare(t_pair)[0] == 0.0
        assert g.L.mi355_group_wait_yolodec(g.h, t, None, C.byref(C.c_uint32(0))) == INV   # null records for a capacity above 0 ...
        m.check(g.wait_yolodec(t))                                                  # ... leave the ticket collectable
        assert g.yolodec_stats() == (1, 1, 1, 1 + net.launches() + 2) and g.yolox_infer_stats()[:3] == (1, 1, 1)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_yolodec(t)                                                       # collected: a double wait is refused
        assert e.value.status == INV
    finally:
        _close(g, [m], [net, raw])
        ctx.free(d_pic)


def test_flush_wait_all_and_destroy_cover_infer_members(ctx):
    import mi355fx
    case = case_of("tiny", 1, 32, 32)
    net = device_net(ctx, case)
    members = [FrameMember(ctx, net, case, k % 3, *LAYOUTS[k % 3]) for k in range(4)]
    g = mi355fx.Group(0)
    try:
        L = net.launches()
        want = [m.lone() for m in members]
        tk = [m.submit(g) for m in members[:2]]
        g.flush()
        assert g.yolodec_stats() == (2, 1, 2, 1 + L + 2)                            # flush launches the queue
        tk += [m.submit(g) for m in members[2:]]
        g.wait_all()                                                                # launches and waits; results stay collectable
        assert g.yolodec_stats() == (4, 2, 2, 2 * (1 + L + 2))
        for m, t, w in zip(members, tk, want):
            m.check(g.wait_yolodec(t), w)
        for m in members:
            m.submit(g)                                                             # two launched and never waited for, two pending
            if m is members[1]:
                g.flush()
        g.close()                                                                   # launches, waits, frees every lane: does not hang
        g = None
        for m, w in zip(members, want):
            m.check(m.lone(), w)                                                    # the net and the device work
    finally:
        _close(g, members, [net])
