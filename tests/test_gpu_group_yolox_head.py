"""GPU tests for yoloxinference's head maps in the decoder queue of the dispatcher (mi355_group_submit_yolox_head, collected with
mi355_group_wait_yolodec): the raw reg / obj / cls maps of INDEPENDENT `yoloxinference ! yoloxtensordec` pipelines as
members of the launch sets the decoded tensors use - one upload of the level tables, two launches (yolox_head_score_jobs_kernel,
yolox_head_nms_jobs_kernel) and the set's one download.

The bar for every head, three ways: the count equal and the records R.same_records to the numpy restatement
(tests/yolox_head_restate.py through tests/yolox_head_cases.py); byte-equal (tobytes()) to the lone mi355_yolox_head_dets_device on
the same maps; and, device against device, equal to what the X decoder of the SAME set makes of the tensor that
mi355_yolox_head_decode_device materialised from those maps (no libm in between)."""
import ctypes as C
import threading

import numpy as np
import pytest

import yolodec_cases as Y
import yolodec_restate as YR
import yolox_head_cases as H
import yolox_head_restate as R

pytestmark = pytest.mark.gpu

POISON = np.float32(30.0)      # a logit in the padding: sigmoid 1, it would survive any threshold


def _same(a, b):
    """R.same_records, a NaN confidence equal to a NaN confidence (the sign and payload of a NaN sigmoid are the hardware's)."""
    a, b = a.copy(), b.copy()
    both = np.isnan(a["confidence"]) & np.isnan(b["confidence"]) if a.shape == b.shape else False
    a["confidence"][both] = b["confidence"][both] = 0
    return R.same_records(a, b)


class HeadMember:
    """One instance's head maps on the device, its settings and its output capacity. form "split": reg, obj and cls of a level in
    regions of their own with `pad` floats of poison behind each; "one": the engine's fused [5 + C, h, w] block per level (obj = reg +
    4 h w, cls = reg + 5 h w), the levels back to back. pitches: what the level structs carry (the queue ignores them)."""

    def __init__(self, c, head, form="split", pad=3, params=None, max_dets=None, ctx=None, pitches=True):
        self.c, self.own, self.head, self.C, self.A = c, ctx or c, head, head.C, head.A
        self.params = head.params if params is None else tuple(float(np.float32(v)) for v in params)
        self.cap = max_dets if max_dets is not None else head.max_dets
        pad = 0 if form == "one" else pad
        parts, plan, at = [], [], 0
        for reg, obj, cls, stride in head.levels:
            hw = reg.shape[1] * reg.shape[2]
            offs = []
            for a in (reg, obj, cls):
                offs.append(at)
                parts += [a.reshape(-1), np.full(pad, POISON, np.float32)]
                at += a.size + pad
            plan.append((offs, hw, reg.shape[1], reg.shape[2], stride))
        self.host = np.concatenate(parts)
        self.d = c.alloc(max(self.host.nbytes, 16))
        c.h2d(self.d, self.host)
        self.levels = [(self.d + 4 * o[0], self.d + 4 * o[1], self.d + 4 * o[2], 16 * hw, 4 * hw, 4 * self.C * hw, h, w, s) for o, hw, h, w, s in plan]
        self.submit_levels = self.levels if pitches else [lv[:3] + (0, 0, 0) + lv[6:] for lv in self.levels]
        self.d_tensor = None
        self._want = None

    def want(self):
        if self._want is None:
            self._want = self.head.expected() if self.params == self.head.params else R.dets(self.head.levels, *np.float32(self.params), decoded=self.head.tensor())
        return self._want

    def submit(self, g):
        return g.submit_yolox_head(self.own, self.submit_levels, self.C, self.params, self.cap)

    def lone(self):
        got, n = self.own.yolox_head_dets_device(self.levels, 1, self.C, [self.params], self.cap, return_counts=True)
        return got[0], n[0]

    def submit_materialised(self, g):
        """The tensor mi355_yolox_head_decode_device makes of these maps, as an X member with the head's settings and capacity."""
        F = 5 + self.C
        if self.d_tensor is None:
            self.d_tensor = self.c.alloc(self.A * F * 4)
            self.own.yolox_head_decode_device(self.levels, 1, self.C, self.d_tensor, self.A * F * 4)
        return g.submit_yolodec(self.own, self.d_tensor, "X", F, self.A, self.params, self.A if self.cap is None else self.cap)

    def check(self, result, lone=None, via=None):
        got, n = result
        lone_got, lone_n = lone or self.lone()
        want = self.want()
        cap = self.A if self.cap is None else self.cap
        name = self.head.name
        assert n == lone_n == len(want), (name, n, lone_n, len(want))               # the full count, even above the capacity
        assert len(got) == min(n, cap), (name, len(got), n, cap)
        assert got.tobytes() == lone_got.tobytes(), name
        assert _same(got, want[:cap]), name
        if via is not None:
            assert via[1] == n and _same(via[0], got), (name, "the X decoder of the same set on the materialised tensor")
        return n

    def free(self):
        self.c.free(self.d)
        if self.d_tensor is not None:
            self.c.free(self.d_tensor)


class TensorMember:
    """A decoded tensor as the decoder queue has always taken it (tests/test_gpu_group_yolodec.py)."""

    def __init__(self, c, case):
        self.c, self.case = c, case
        self.d = c.alloc(max(case.data.nbytes, 16))
        c.h2d(self.d, case.data)

    def submit(self, g):
        return g.submit_yolodec(self.c, self.d, self.case.layout, self.case.F, self.case.N, self.case.params, self.case.max_dets)

    def check(self, result, lone=None, via=None):
        got, n = result
        lone_got, lone_n = self.c.yolodec_device(self.d, self.case.F * self.case.N * 4, 1, self.case.layout, self.case.F, self.case.N, [self.case.params],
                                                 self.case.max_dets, return_counts=True)
        assert n == lone_n[0] == len(self.case.expected()) and got.tobytes() == lone_got[0].tobytes(), self.case.name
        assert YR.same_records(got, self.case.expected()), self.case.name
        return n

    def free(self):
        self.c.free(self.d)


def _tensor(k, layout, F, N):
    rng = np.random.default_rng(900 + k)
    params = (float(rng.uniform(0.3, 0.6)), float(rng.uniform(0.3, 0.6)), float(rng.uniform(0.1, 0.8)))
    return Y.Case("t%d_%s_F%d_N%d" % (k, layout, F, N), layout, Y.synth(7000 + k, layout, F, N, frac=0.3), params)


def _free(g, members):
    if g is not None:
        g.close()
    for m in members:
        m.free()


def _run_with_materialised(g, heads, reverse=False):
    """Each head and, behind them in the SAME set, its materialised tensor as an X member; waits, checks all three ways."""
    tk = [m.submit(g) for m in heads]
    tv = [m.submit_materialised(g) for m in heads]
    order = list(reversed(range(len(heads)))) if reverse else list(range(len(heads)))
    res, via = {}, {}
    for k in order:
        via[k] = g.wait_yolodec(tv[k])
        res[k] = g.wait_yolodec(tk[k])
    return [m.check(res[k], via=via[k]) for k, m in enumerate(heads)]


@pytest.mark.parametrize("set_name", list(H.LEVEL_SETS))
def test_shapes_alone_in_a_set(ctx, set_name):
    """one: A = 1; row65: one partial tile; boundary255: a level whose last tile holds 255 lanes, then a 2-candidate level; eight:
    eight levels. Alone in a set (one upload, two launches), then once more beside the materialised tensor."""
    import mi355fx
    members = [HeadMember(ctx, H.shape_head(set_name, Cn), form, pad) for Cn, form, pad in ((1, "split", 3), (80, "one", 0))]
    g = mi355fx.Group(0)
    try:
        for k, m in enumerate(members):
            t = m.submit(g)
            assert g.yolodec_stats() == (2 * k, 2 * k, 1 if k else 0, 4 * k) and g.yolox_head_stats() == (2 * k, 2 * k, 2 * k, 4 * k)   # nothing goes out before a wait
            m.check(g.wait_yolodec(t))
            assert g.yolodec_stats() == (2 * k + 1, 2 * k + 1, 1, 4 * k + 2)        # a head counts as a tensor; its two launches
            assert g.yolox_head_stats() == (2 * k + 1, 2 * k + 1, 2 * k + 1, 4 * k + 2)   # one upload
            t = m.submit(g)
            m.check(g.wait_yolodec(t))                                              # the same head again: counters and keys are clean
        g.close()
        g = mi355fx.Group(0)
        _run_with_materialised(g, members)
        assert g.yolodec_stats() == (4, 1, 4, 4) and g.yolox_head_stats() == (2, 1, 1, 2)   # X score, tensor NMS, head score, head NMS
    finally:
        _free(g, members)


@pytest.mark.parametrize("reverse", [False, True])
def test_one_mixed_set(ctx, reverse):
    """A V8 tensor, an X tensor - the materialised tensor of the first head, so device stands against device inside the set - and four
    heads that differ in level set, C, form, settings and capacity, submitted in both orders: one set, the tensors' three launches and
    the heads' two, one upload."""
    import mi355fx
    heads = [HeadMember(ctx, H.shape_head("boundary255", 80), "one", params=(0.45, 0.4, 0.3)),
             HeadMember(ctx, H.shape_head("eight", 2), "split", 1, max_dets=5),
             HeadMember(ctx, H.shape_head("three_square", 128), "split", 0, params=(0.3, 0.55, 0.7), pitches=False),
             HeadMember(ctx, H.shape_head("row65", 1), "one", params=(0.6, 0.2, 0.1), max_dets=1000)]
    v8 = TensorMember(ctx, _tensor(1, "V8", 84, 300))
    g = mi355fx.Group(0)
    try:
        assert len({m.C for m in heads}) == 4 and len({m.params for m in heads}) == 4
        calls = [v8.submit, heads[0].submit_materialised] + [m.submit for m in heads]
        who = [v8, None] + heads
        order = list(reversed(range(6))) if reverse else list(range(6))
        tk = {k: calls[k](g) for k in order}
        assert g.yolodec_stats() == (0, 0, 0, 0) and g.yolox_head_stats() == (0, 0, 0, 0)
        res = {k: g.wait_yolodec(tk[k]) for k in order}
        assert g.yolodec_stats() == (6, 1, 6, 5)
        assert g.yolox_head_stats() == (4, 1, 1, 2)
        counts = [who[k].check(res[k], via=res[1] if k == 2 else None) for k in (0, 2, 3, 4, 5)]
        assert all(c > 0 for c in counts) and counts[2] > 5                         # (the capacity of 5 truncates)
    finally:
        _free(g, heads + [v8])


def test_special_heads_share_one_set(ctx):
    """Class ties of the sigmoid, non-finite values, the objectness drop with zero and some survivors, the global sort path, a count
    above the capacity and max_dets = 0, each beside its materialised tensor."""
    import mi355fx
    tie, classes = H.tie_head()
    objdrop, kept = H.objdrop_head()
    none = H.random_head("no_survivor", 6100, [(3, 5), (2, 3)], (8, 16), 4, params=(0.5, 0.5, 0.45), obj_shift=-40.0)
    heads = [HeadMember(ctx, tie), HeadMember(ctx, H.nonfinite_head(), "one"), HeadMember(ctx, objdrop), HeadMember(ctx, none), HeadMember(ctx, H.sort_head(), "one"),
             HeadMember(ctx, H.trunc_head(7)), HeadMember(ctx, H.trunc_head(0))]
    g = mi355fx.Group(0)
    try:
        counts = _run_with_materialised(g, heads, reverse=True)
        assert g.yolodec_stats() == (14, 1, 14, 4) and g.yolox_head_stats() == (7, 1, 1, 2)
        assert counts[0] == len(classes) and counts[1] == 8 and counts[2] == len(kept) and counts[3] == 0
        assert 4096 < heads[4].A and counts[4] > 0 and counts[5] > 7 and counts[6] == counts[5]
        # max_dets = 0 with null records, through the C entry itself
        t = heads[6].submit(g)
        n = C.c_uint32(77)
        assert g.L.mi355_group_wait_yolodec(g.h, t, None, C.byref(n)) == 0 and n.value == counts[6]
        # ... and null records with max_dets > 0 are refused; the result stays collectable
        t = heads[5].submit(g)
        assert g.L.mi355_group_wait_yolodec(g.h, t, None, C.byref(n)) == mi355fx.ERR_INVALID_ARG
        heads[5].check(g.wait_yolodec(t))
    finally:
        _free(g, heads)


def test_the_three_maps_of_a_level_in_one_allocation(ctx):
    """Every level a fused [5 + C, h, w] block: obj and cls are offsets into reg's allocation."""
    import mi355fx
    heads = [HeadMember(ctx, H.shape_head(name, Cn), "one") for name, Cn in (("three_small", 80), ("boundary255", 1), ("eight", 80), ("three_square", 2))]
    g = mi355fx.Group(0)
    try:
        for m in heads:
            for reg, obj, cls, _, _, _, h, w, _ in m.levels:
                assert obj == reg + 16 * h * w and cls == reg + 20 * h * w
        counts = _run_with_materialised(g, heads)
        assert g.yolodec_stats() == (8, 1, 8, 4) and g.yolox_head_stats() == (4, 1, 1, 2)
        assert sum(counts) > 10
    finally:
        _free(g, heads)


def test_a_full_level_table_two_sets_and_a_growing_slab(ctx):
    """32 heads of eight levels: 256 level jobs, the table's maximum, in the set the 32nd submit fills. The 33rd head goes to a second
    set and has room for more records than the whole first set, so every slab grows under the first set's uncollected results. Waits
    come in reverse order."""
    import mi355fx
    shapes = H.LEVEL_SETS["eight"]
    small = [HeadMember(ctx, H.random_head("full_%d" % k, 8000 + 37 * k, shapes, H.STRIDES, (1, 3, 9)[k % 3], params=(0.3, 0.3, 0.6)), ("split", "one")[k % 2], k % 3)
             for k in range(32)]
    big = HeadMember(ctx, H.sort_head())
    g = mi355fx.Group(0)
    try:
        assert sum(len(m.levels) for m in small) == 256 == 32 * mi355fx.YOLOX_LEVELS_MAX
        tk = [m.submit(g) for m in small]
        assert g.yolodec_stats() == (32, 1, 32, 2) and g.yolox_head_stats() == (32, 1, 1, 2)    # the 32nd submit filled a set
        tb = big.submit(g)
        assert g.yolodec_stats() == (32, 1, 32, 2)
        n_big = big.check(g.wait_yolodec(tb))
        assert g.yolodec_stats() == (33, 2, 32, 4) and g.yolox_head_stats() == (33, 2, 2, 4)
        assert n_big > 0 and big.A > sum(m.A for m in small)                        # its slots alone exceed the first set's whole result slab
        res = {k: g.wait_yolodec(tk[k]) for k in reversed(range(32))}
        counts = [m.check(res[k]) for k, m in enumerate(small)]
        assert sum(counts) > 100 and len(set(counts)) > 4
        assert g.yolodec_stats() == (33, 2, 32, 4)
    finally:
        _free(g, small + [big])


def test_counters_and_keys_stay_clean_over_intervals(ctx):
    """Big, small, medium, small, big head intervals on one group, a tensor-only interval between them: a survivor counter that was
    not left at zero, or keys or tables of an earlier interval read again, change a count. The tensor-only intervals launch what they
    always did and upload nothing."""
    import mi355fx
    big = [HeadMember(ctx, H.sort_head(), "one"), HeadMember(ctx, H.shape_head("three_square", 80))]
    small = [HeadMember(ctx, H.shape_head("one", 1)), HeadMember(ctx, H.kat_head()[0]), HeadMember(ctx, H.shape_head("three_small", 2), "one")]
    medium = [HeadMember(ctx, h, ("split", "one")[k % 2]) for k, h in enumerate(H.batch_heads(4))]
    tensors = [TensorMember(ctx, _tensor(10, "V8", 20, 1000)), TensorMember(ctx, _tensor(11, "X", 9, 257))]
    g = mi355fx.Group(0)
    try:
        lone = {m: m.lone() for m in big + small + medium}
        for k, members in enumerate((big, small, medium, small, big)):
            tk = [m.submit(g) for m in members]
            for m, t in zip(members, tk):
                m.check(g.wait_yolodec(t), lone[m])
            assert g.yolox_head_stats() == (sum(len(s) for s in (big, small, medium, small, big)[:k + 1]), k + 1, k + 1, 2 * (k + 1))
            before, heads_before = g.yolodec_stats(), g.yolox_head_stats()
            tk = [m.submit(g) for m in tensors]
            for m, t in zip(tensors, tk):
                m.check(g.wait_yolodec(t))
            after = g.yolodec_stats()
            assert (after[0] - before[0], after[1] - before[1], after[3] - before[3]) == (2, 1, 3)   # V8 score, X score, NMS: as ever
            assert g.yolox_head_stats() == heads_before
    finally:
        _free(g, big + small + medium + tensors)


def test_refusals_and_ticket_classes(ctx):
    import mi355fx
    m = HeadMember(ctx, H.shape_head("three_small", 2))
    lv = m.levels
    pic = np.random.default_rng(3).integers(0, 256, 64 * 48 * 4, dtype=np.uint8)
    d_pic, d_out = ctx.alloc(pic.nbytes), ctx.alloc(pic.nbytes)
    ctx.h2d(d_pic, pic)
    g = mi355fx.Group(0)
    P = (0.5, 0.5, 0.5)
    INV, UNS = mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED

    def level(k, **kw):
        names = ("reg", "obj", "cls", "reg_pitch", "obj_pitch", "cls_pitch", "h", "w", "stride", "reserved")
        q = list(lv[k]) + [0]
        for name, v in kw.items():
            q[names.index(name)] = v
        return tuple(q)

    try:
        shape_cases = [
            ([], 2, INV),                                                            # no level
            (lv, 0, INV),                                                            # no class
            (lv * 3, 2, UNS),                                                        # nine levels
            (lv, 1025, UNS),                                                         # more than 1029 fields
            ([lv[0], level(1, h=0), lv[2]], 2, INV),
            ([lv[0], level(1, w=0), lv[2]], 2, INV),
            ([lv[0], lv[1], level(2, stride=0)], 2, INV),
            ([lv[0], lv[1], level(2, reserved=1)], 2, INV),
            ([level(0, stride=65537), lv[1], lv[2]], 2, UNS),
            ([level(0, h=256, w=256, reg_pitch=1 << 20, obj_pitch=1 << 18, cls_pitch=1 << 19), lv[1], lv[2]], 2, UNS),   # more than 65536 candidates
            ([level(0, reg=None), lv[1], lv[2]], 2, INV),
            ([lv[0], level(1, obj=None), lv[2]], 2, INV),
            ([lv[0], lv[1], level(2, cls=None)], 2, INV),
            ([lv[0], level(1, cls=lv[1][2] + 2), lv[2]], 2, INV),                    # a misaligned map
        ]
        for levels, Cn, status in shape_cases:
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.submit_yolox_head(ctx, levels, Cn, P, 10)
            assert e.value.status == status, (levels, Cn)
            # the checker's own status for the same levels and one tensor, with an output pitch that fits
            A = sum(q[6] * q[7] for q in levels)
            assert mi355fx.selftest_yolox_head_check(levels, 1, Cn, A * (5 + Cn) * 4) == status, (levels, Cn)
        bad = [
            lambda: g.submit_yolox_head(ctx, None, 2, P, 10, n_levels=3),            # null levels
            lambda: g.submit_yolox_head(ctx, lv, 2, None, 10),                       # null settings
            lambda: g.submit_yolox_head(None, lv, 2, P, 10),                         # null context
            lambda: g.wait_yolodec(0),                                               # unknown tickets
            lambda: g.wait_yolodec(12345),
        ]
        for call in bad:
            with pytest.raises(mi355fx.Mi355Error) as e:
                call()
            assert e.value.status == INV
        arr, p = mi355fx._yolox_levels(lv), C.byref(mi355fx.YoloParams(*P))
        t64 = C.c_uint64(0)
        assert g.L.mi355_group_submit_yolox_head(g.h, ctx.h, arr, 3, 2, p, 10, None) == INV          # null ticket
        assert g.L.mi355_group_submit_yolox_head(None, ctx.h, arr, 3, 2, p, 10, C.byref(t64)) == INV  # null group
        assert g.L.mi355_group_yolox_head_stats(g.h, None) == INV and g.L.mi355_group_yolox_head_stats(None, (C.c_uint64 * 4)()) == INV
        # the lone entry refuses the same shapes with the same status
        for levels, Cn, status in (shape_cases[2], shape_cases[4], shape_cases[9], shape_cases[10]):
            with pytest.raises(mi355fx.Mi355Error) as e:
                ctx.yolox_head_dets_device(levels, 1, Cn, [P])
            assert e.value.status == status
        assert g.yolodec_stats() == (0, 0, 0, 0) and g.yolox_head_stats() == (0, 0, 0, 0)
        g.flush()
        assert g.yolodec_stats() == (0, 0, 0, 0) and g.yolox_head_stats() == (0, 0, 0, 0)   # a refused submit queued nothing
        t = m.submit(g)
        # tickets of the other queues are refused by the decoder queue's wait and stay collectable there
        t_pair = g.submit_compare(ctx, d_pic, d_pic, 256, 64, 48, "RGBA", 5)
        t_cd = g.submit_colordetect(ctx, d_pic, pic.nbytes, "RGBA", 10, 2)
        t_hd = g.submit_hsvdetect(ctx, d_pic, 256, "RGBx", d_out, 256, "RGBA", 64, 48, (120.0, 40.0, 0.8, 0.5, 0.7, 0.6))
        for other in (t_pair, t_cd, t_hd):
            with pytest.raises(mi355fx.Mi355Error) as e:
                g.wait_yolodec(other)
            assert e.value.status == INV
        # ... and the reverse: a head ticket is a decoder ticket
        for refuse in (g.wait, lambda tt: g.order_after(ctx, tt), g.wait_compare, g.wait_colordetect, g.wait_hsvdetect, g.wait_handdec):
            with pytest.raises(mi355fx.Mi355Error) as e:
                refuse(t)
            assert e.value.status == INV
        assert g.yolodec_stats() == (0, 0, 0, 0)
        assert g.wait_compare(t_pair)[0] == 0.0
        assert 1 <= len(g.wait_colordetect(t_cd)) <= 2
        g.wait_hsvdetect(t_hd)
        assert g.yolodec_stats() == (0, 0, 0, 0) and g.yolox_head_stats() == (0, 0, 0, 0)   # the other queues' launches are theirs
        m.check(g.wait_yolodec(t))                                                  # the first valid submit after the refusals is right
        assert g.yolodec_stats() == (1, 1, 1, 2) and g.yolox_head_stats() == (1, 1, 1, 2)
        with pytest.raises(mi355fx.Mi355Error) as e:
            g.wait_yolodec(t)                                                       # collected: a double wait is refused
        assert e.value.status == INV
        assert g.yolodec_stats() == (1, 1, 1, 2) and g.yolox_head_stats() == (1, 1, 1, 2)
    finally:
        _free(g, [m])
        ctx.free(d_pic)
        ctx.free(d_out)


def test_the_maps_are_read_after_what_their_stream_held(ctx):
    """The maps are written by a device copy on the member's stream immediately before the submit, behind four 64 MiB copies that
    keep the stream busy, with no synchronisation: the set, on the queue's own stream, must wait for it."""
    import mi355fx
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3
    shapes, strides = [(16, 16), (8, 8), (4, 4)], (8, 16, 32)
    real = H.random_head("stream_real", 6600, shapes, strides, 5, params=(0.4, 0.45, 0.45))
    decoy = H.random_head("stream_decoy", 6700, shapes, strides, 5, params=real.params)
    m = HeadMember(ctx, decoy)                                                      # the device maps hold the decoy for now
    r = HeadMember(ctx, real)                                                       # the same layout: its buffer is the staging copy
    filler = 64 << 20
    a, b = ctx.alloc(filler), ctx.alloc(filler)
    g = mi355fx.Group(0)
    try:
        assert m.host.nbytes == r.host.nbytes
        old = m.lone()
        assert old[1] == len(decoy.expected())
        for _ in range(4):
            assert hip.hipMemcpyAsync(b, a, filler, D2D, ctx.stream) == 0
        assert hip.hipMemcpyAsync(m.d, r.d, r.host.nbytes, D2D, ctx.stream) == 0
        t = m.submit(g)
        got = g.wait_yolodec(t)
        m.head, m._want = real, None                                                # what the maps hold now
        m.check(got)
        assert got[0].tobytes() != old[0].tobytes()
    finally:
        _free(g, [m, r])
        for p in (a, b):
            ctx.free(p)


def test_rendezvous_threads(mi355lib):
    """Eight instances on eight threads x 10 intervals, each with its own context, level set and C, submitting and waiting at once
    (what transform_ip does); rendezvous 8 with a 2 ms linger. One thread sits out every third interval."""
    import mi355fx
    n, rounds = 8, 10
    ctxs = [mi355fx.Context(0) for _ in range(n)]
    names = list(H.LEVEL_SETS)
    members = [HeadMember(ctxs[0], H.shape_head(names[s % len(names)], (80, 1, 2, 128)[s % 4]), ("split", "one")[s % 2], ctx=c) for s, c in enumerate(ctxs)]
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
        st, hs = g.yolodec_stats(), g.yolox_head_stats()
        assert sum(seen) == total == st[0] == hs[0] and st[2] <= n and rounds <= st[1] <= total
        assert hs[1] == hs[2] == st[1] and hs[3] == st[3] == 2 * st[1]              # every set: one upload, two launches
    finally:
        _free(g, members)
        for c in ctxs:
            c.close()


def test_flush_wait_all_and_destroy_cover_heads(ctx):
    import mi355fx
    members = [HeadMember(ctx, h, ("split", "one")[k % 2]) for k, h in enumerate(H.batch_heads(4, seed=1300))]
    g = mi355fx.Group(0)
    try:
        tk = [m.submit(g) for m in members[:2]]
        g.flush()
        assert g.yolodec_stats() == (2, 1, 2, 2) and g.yolox_head_stats() == (2, 1, 1, 2)   # flush launches the queue
        tk += [m.submit(g) for m in members[2:]]
        g.wait_all()                                                                # launches and waits; results stay collectable
        assert g.yolodec_stats() == (4, 2, 2, 4) and g.yolox_head_stats() == (4, 2, 2, 4)
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
