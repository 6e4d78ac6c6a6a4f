"""The YOLOX head decoder on the GPU: mi355_yolox_head_decode_device bit-equal to the numpy restatement
(tests/yolox_head_restate.py; NaN == NaN), the fused mi355_yolox_head_dets_device / mi355_yolox_head_dets record for record equal to
yolodec_restate.decode of the restated tensor AND to mi355_yolodec_tensors_device run on the device-materialised tensor (device
against device: no libm in between), and mi355_yolox_input_frames_device byte-exact. Cases: tests/yolox_head_cases.py."""
import numpy as np
import pytest

import yolox_head_cases as H
import yolox_head_restate as R

pytestmark = pytest.mark.gpu

POISON = np.float32(30.0)      # a logit in the padding: sigmoid 1, it would survive any threshold


class DeviceHeads:
    """n heads of one shape on the device. form "split": reg, obj and cls of a level in regions of their own, each with its own pitch
    (pad_floats of poison behind every map); form "one": the engine's fused [5 + C, h, w] block per level and tensor - obj = reg +
    4 h w, cls = reg + 5 h w, equal pitches."""

    def __init__(self, ctx, heads, form="split", pad_floats=0):
        self.ctx, self.n, self.C, self.A = ctx, len(heads), heads[0].C, heads[0].A
        C = self.C
        plan, at = [], 0                       # per level: float offsets of reg, obj, cls and their pitches in floats
        for reg, _, _, stride in heads[0].levels:
            hw = reg.shape[1] * reg.shape[2]
            if form == "one":
                pitch = (5 + C) * hw + pad_floats
                plan.append((at, at + 4 * hw, at + 5 * hw, pitch, pitch, pitch, reg.shape[1], reg.shape[2], stride))
                at += pitch * self.n
            else:
                pr, po, pc = 4 * hw + pad_floats, hw + pad_floats, C * hw + pad_floats
                plan.append((at, at + pr * self.n, at + (pr + po) * self.n, pr, po, pc, reg.shape[1], reg.shape[2], stride))
                at += (pr + po + pc) * self.n
        buf = np.full(at, POISON, np.float32)
        for t, head in enumerate(heads):
            for (o_r, o_o, o_c, p_r, p_o, p_c, h, w, _), (reg, obj, cls, _) in zip(plan, head.levels):
                hw = h * w
                buf[o_r + t * p_r: o_r + t * p_r + 4 * hw] = reg.reshape(-1)
                buf[o_o + t * p_o: o_o + t * p_o + hw] = obj.reshape(-1)
                buf[o_c + t * p_c: o_c + t * p_c + C * hw] = cls.reshape(-1)
        self.d = ctx.alloc(max(buf.nbytes, 16))
        ctx.h2d(self.d, buf)
        self.levels = [(self.d + 4 * o_r, self.d + 4 * o_o, self.d + 4 * o_c, 4 * p_r, 4 * p_o, 4 * p_c, h, w, s) for o_r, o_o, o_c, p_r, p_o, p_c, h, w, s in plan]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.free(self.d)

    def dets(self, params, max_dets=None):
        return self.ctx.yolox_head_dets_device(self.levels, self.n, self.C, params, max_dets, return_counts=True)

    def materialise(self, pad_floats=0):
        """-> (the n decoded tensors read back, device pointer, pitch in bytes); the caller frees the pointer."""
        F = 5 + self.C
        pitch = (self.A * F + pad_floats) * 4
        out = np.full(self.n * pitch // 4, np.float32(7e30), np.float32)
        d_out = self.ctx.alloc(max(out.nbytes, 16))
        self.ctx.h2d(d_out, out)
        self.ctx.yolox_head_decode_device(self.levels, self.n, self.C, d_out, pitch)
        self.ctx.d2h(out, d_out)
        rows = out.reshape(self.n, pitch // 4)
        assert (rows[:, self.A * F:] == np.float32(7e30)).all()          # nothing written behind a tensor
        return [rows[t, :self.A * F].reshape(self.A, F) for t in range(self.n)], d_out, pitch


def _same(a, b):
    """R.same_records, a NaN confidence equal to a NaN confidence (the sign and payload of a NaN sigmoid are the hardware's)."""
    a, b = a.copy(), b.copy()
    both = np.isnan(a["confidence"]) & np.isnan(b["confidence"]) if a.shape == b.shape else False
    a["confidence"][both] = b["confidence"][both] = 0
    return R.same_records(a, b)


def _check_records(got, n, head, what):
    want = head.expected()
    cap = head.A if head.max_dets is None else head.max_dets
    assert n == len(want), (head.name, what, n, len(want))                # the full count, even above the capacity
    assert _same(got, want[:cap]), (head.name, what)


def _host_levels(head):
    return [(reg, obj, cls, s) for reg, obj, cls, s in head.levels]


def _everything(ctx, head, form="split", pad_floats=0):
    """One head through every entry point: materialised tensor, fused device form, the X decoder on the device tensor, host form."""
    with DeviceHeads(ctx, [head], form, pad_floats) as D:
        tensors, d_t, pitch = D.materialise(pad_floats)
        try:
            assert R.same_tensor(tensors[0], head.tensor()), (head.name, "materialised tensor")
            got, n = D.dets([head.params], head.max_dets)
            _check_records(got[0], n[0], head, "fused device form")
            via, n_via = ctx.yolodec_device(d_t, pitch, 1, "X", 5 + head.C, head.A, [head.params], head.max_dets, return_counts=True)
            assert n_via[0] == n[0] and _same(via[0], got[0]), (head.name, "X decoder on the device tensor")
        finally:
            ctx.free(d_t)
    host, n_host = ctx.yolox_head_dets(_host_levels(head), head.params, head.max_dets, return_count=True)
    assert n_host == n[0] and _same(host, got[0]), (head.name, "host form")
    return got[0]


@pytest.mark.parametrize("set_name", list(H.LEVEL_SETS))
def test_shapes_match_the_restatement(ctx, set_name):
    for k, C in enumerate(H.CLASSES):
        form, pad = [("split", 0), ("split", 3), ("one", 0), ("one", 5)][(k + list(H.LEVEL_SETS).index(set_name)) % 4]
        _everything(ctx, H.shape_head(set_name, C), form, pad)


@pytest.mark.parametrize("form,pad", [("split", 0), ("split", 7), ("one", 0), ("one", 2)])
def test_padded_pitches_and_the_one_allocation_form(ctx, form, pad):
    got = _everything(ctx, H.shape_head("boundary255", 80), form, pad)
    assert 0 < len(got) < 257


def test_known_answers_by_hand(ctx):
    head, rows = H.kat_head()
    got = _everything(ctx, head)
    assert [int(d["candidate"]) for d in got] == [c for c, _ in rows]
    assert [(int(d["x"]), int(d["y"]), int(d["width"]), int(d["height"]), float(d["confidence"])) for d in got] == [(16, 6, 8, 8, 0.5), (16, 28, 16, 16, 0.5),
                                                                                                                     (32, -8, 32, 32, 0.5)]


def test_unfused_add_and_multiply(ctx):
    _everything(ctx, H.unfused_head())


def test_class_ties_of_the_sigmoid(ctx):
    head, classes = H.tie_head()
    got = _everything(ctx, head)
    assert {int(d["candidate"]): int(d["class_id"]) for d in got} == dict(enumerate(classes))


def test_objectness_drop_before_the_classes(ctx):
    head, kept = H.objdrop_head()
    got = _everything(ctx, head)
    assert sorted(int(d["candidate"]) for d in got) == kept            # 0 and 3: just below box_thr; 2: obj = NaN stays


def test_non_finite_values(ctx):
    got = _everything(ctx, H.nonfinite_head())
    assert len(got) == 8


@pytest.mark.parametrize("n_tensors", [1, 3, 33])
def test_batches_with_their_own_settings_equal_lone_calls(ctx, n_tensors):
    heads = H.batch_heads(n_tensors)
    params = [H.batch_settings(k) for k in range(n_tensors)]
    with DeviceHeads(ctx, heads, "split", 3) as D:
        got, n = D.dets(params)
        tensors, d_t, _ = D.materialise()
        ctx.free(d_t)
    for k, head in enumerate(heads):
        assert R.same_tensor(tensors[k], head.tensor()), k
        want = R.dets(head.levels, *np.float32(params[k]), decoded=head.tensor())
        with DeviceHeads(ctx, [head]) as L:
            lone, n_lone = L.dets([params[k]])
        assert n[k] == len(want) == n_lone[0] and R.same_records(got[k], want) and R.same_records(lone[0], want), k
    assert len({len(g) for g in got}) > 1 or n_tensors == 1


def test_batch_with_all_dropped_and_all_kept_tensors(ctx):
    heads = H.batch_heads(5, seed=700)
    params = [(0.5, 0.45, 0.45), (0.5, 5.0, 0.45), (0.0, 0.0, 2.0), (5.0, 0.0, 0.45), (0.5, 0.45, 0.45)]   # [2]: every candidate, NMS off
    with DeviceHeads(ctx, heads, "one", 1) as D:
        got, n = D.dets(params)
    assert n[1] == 0 and n[3] == 0 and n[2] == heads[2].A and 0 < n[0] < heads[0].A
    for k, head in enumerate(heads):
        assert R.same_records(got[k], R.dets(head.levels, *np.float32(params[k]), decoded=head.tensor())), k


def test_the_same_call_twice_and_big_then_small(ctx):
    """A survivor counter that is not left at zero would append the second call's keys behind the first call's."""
    big, small = H.sort_head(), H.shape_head("three_small", 2)
    with DeviceHeads(ctx, [big]) as B, DeviceHeads(ctx, [small]) as S:
        for D, head in ((B, big), (B, big), (S, small), (S, small), (B, big)):
            got, n = D.dets([head.params])
            _check_records(got[0], n[0], head, "sequence")
        # the tensor decoder shares the scratch and its counters
        t = small.tensor()
        via = ctx.yolodec(t, "X", small.params)
        assert R.same_records(via, small.expected())
        got, n = S.dets([small.params])
        _check_records(got[0], n[0], small, "after the tensor decoder")


def test_global_scratch_sort_path(ctx):
    head = H.sort_head()
    assert head.A == 5376
    got = _everything(ctx, head)
    assert 0 < len(got) < head.A


@pytest.mark.parametrize("cap", [0, 1, 7])
def test_max_dets_below_the_count(ctx, cap):
    head = H.trunc_head(cap)
    assert len(head.expected()) > 7
    _everything(ctx, head)


def test_refused_calls_leave_the_context_usable(ctx):
    import mi355fx
    head = H.shape_head("three_small", 2)
    with DeviceHeads(ctx, [head]) as D:
        bad = [list(lv) for lv in D.levels]
        bad[1][3] -= 4                                                   # a reg pitch below the map
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.yolox_head_dets_device([tuple(lv) for lv in bad], 1, head.C, [head.params])
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.yolox_head_dets_device(D.levels * 3, 1, head.C, [head.params])      # nine levels
        assert e.value.status == mi355fx.ERR_UNSUPPORTED
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.yolox_head_decode_device(D.levels, 1, head.C, None, head.A * (5 + head.C) * 4)
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        got, n = D.dets([head.params])
        _check_records(got[0], n[0], head, "after the refusals")


@pytest.mark.parametrize("height", [1, 3])
@pytest.mark.parametrize("width", [1, 31, 33, 65])
def test_input_frames_byte_exact(ctx, width, height):
    for n_frames, pad in ((1, 0), (3, 0), (1, 5), (3, 2)):
        buf, pitch, stride = H.frames(width * 10 + height + n_frames, n_frames, width, height, pad)
        out_pitch = (3 * width * height + (3 if pad else 0)) * 4
        out = np.full(n_frames * out_pitch // 4, np.float32(-1.0), np.float32)
        d_in, d_out = ctx.alloc(max(buf.nbytes, 16)), ctx.alloc(max(out.nbytes, 16))
        try:
            ctx.h2d(d_in, buf)
            ctx.h2d(d_out, out)
            ctx.yolox_input_frames_device(d_in, pitch, stride, n_frames, width, height, d_out, out_pitch)
            ctx.d2h(out, d_out)
        finally:
            ctx.free(d_in)
            ctx.free(d_out)
        rows = out.reshape(n_frames, out_pitch // 4)
        for f in range(n_frames):
            want = R.input_tensor(buf[f * pitch:], stride, width, height)
            assert (rows[f, :3 * width * height].view(np.uint32) == want.reshape(-1).view(np.uint32)).all(), (width, height, n_frames, pad, f)
            assert (rows[f, 3 * width * height:] == np.float32(-1.0)).all()
