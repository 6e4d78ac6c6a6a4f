"""yolov8tensordec2 / yoloxtensordec on the GPU: mi355_yolodec_tensor and mi355_yolodec_tensors_device against the numpy
restatement (tests/yolodec_restate.py) on every case of tests/yolodec_cases.py - every record field bit-equal (the
four f32 box fields with NaN == NaN), the counts equal - and the batch, pitch, repeat and refusal behaviour of the entry points."""
import numpy as np
import pytest

import yolodec_cases as Y
import yolodec_restate as R

pytestmark = pytest.mark.gpu


def _check(got, n, case, what):
    want = case.expected()
    cap = case.N if case.max_dets is None else case.max_dets
    assert n == len(want), (case.name, what, n, len(want))                # the full count, even above the capacity
    assert R.same_records(got, want[:cap]), (case.name, what)             # a prefix of the untruncated answer


def _device_call(ctx, tensors, layout, F, N, params, max_dets=None, pad_bytes=0):
    """tensors of one shape side by side at a pitch of F * N * 4 + pad_bytes -> (record arrays, counts)"""
    pitch = F * N * 4 + pad_bytes
    buf = np.full(pitch * len(tensors) // 4, np.float32(7e30), np.float32)   # what lies in the padding would survive any threshold
    for k, t in enumerate(tensors):
        buf[k * pitch // 4: k * pitch // 4 + F * N] = t.reshape(-1)
    d = ctx.alloc(max(buf.nbytes, 16))
    try:
        ctx.h2d(d, buf)
        return ctx.yolodec_device(d, pitch, len(tensors), layout, F, N, params, max_dets, return_counts=True)
    finally:
        ctx.free(d)


@pytest.mark.parametrize("name", Y.GROUPS)
def test_cases_match_the_restatement(ctx, name):
    for case in Y.group(name):
        got, n = ctx.yolodec(case.data, case.layout, case.params, case.max_dets, return_count=True)
        _check(got, n, case, "host tensor")
        got, n = _device_call(ctx, [case.data], case.layout, case.F, case.N, [case.params], case.max_dets)
        _check(got[0], n[0], case, "device tensor")


def test_known_answers_by_hand(ctx):
    for case, rows, confs in Y.kats():
        got = ctx.yolodec(case.data, case.layout, case.params)
        assert [(int(d["x"]), int(d["y"]), int(d["width"]), int(d["height"]), int(d["class_id"]), int(d["candidate"])) for d in got] == rows, case.name
        assert [d["confidence"].view(np.uint32) for d in got] == [np.float32(c).view(np.uint32) for c in confs], case.name


def _settings(k):
    rng = np.random.default_rng(40 + k)
    return (float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.3, 0.8)), float(rng.uniform(0.1, 0.8)))


@pytest.mark.parametrize("layout", ["V8", "X"])
@pytest.mark.parametrize("n_tensors", [1, 3, 33])
def test_batches_with_their_own_settings_equal_lone_calls(ctx, layout, n_tensors):
    F, N = (13, 333) if layout == "V8" else (14, 333)
    tensors = [Y.synth(300 + k, layout, F, N, frac=0.4) for k in range(n_tensors)]
    params = [_settings(k) for k in range(n_tensors)]
    got, n = _device_call(ctx, tensors, layout, F, N, params)
    for k in range(n_tensors):
        lone = ctx.yolodec(tensors[k], layout, params[k])
        want = R.decode(tensors[k], layout, *np.float32(params[k]))
        assert n[k] == len(want) and R.same_records(got[k], want) and R.same_records(lone, want), k
    assert len({len(g) for g in got}) > 1 or n_tensors == 1


@pytest.mark.parametrize("layout", ["V8", "X"])
def test_batch_with_empty_and_full_tensors(ctx, layout):
    F, N = 9, 700
    tensors = [Y.synth(500 + k, layout, F, N, frac=0.3) for k in range(5)]
    params = [(0.5, 0.45, 0.45), (0.5, 5.0, 0.45), (0.0, 0.0, 2.0), (5.0, 5.0, 0.45), (0.5, 0.45, 0.45)]   # [2]: every candidate, NMS off
    got, n = _device_call(ctx, tensors, layout, F, N, params)
    assert n[1] == 0 and n[3] == 0 and n[2] == N and 0 < n[0] < N
    for k in range(5):
        assert R.same_records(got[k], R.decode(tensors[k], layout, *np.float32(params[k]))), k


@pytest.mark.parametrize("layout", ["V8", "X"])
def test_pitch_larger_than_the_tensor(ctx, layout):
    F, N = 11, 257
    tensors = [Y.synth(600 + k, layout, F, N, frac=0.4) for k in range(4)]
    params = [(0.4, 0.45, 0.5)] * 4
    got, n = _device_call(ctx, tensors, layout, F, N, params, pad_bytes=4 * 37)
    for k in range(4):
        assert R.same_records(got[k], R.decode(tensors[k], layout, *np.float32(params[k]))), k


def test_repeats_and_big_then_small_on_one_context(ctx):
    big = Y.group("sort_switch")[1]              # 4096 candidates, all surviving
    small = Y.group("random")[3]
    tiny = Y.kats()[0][0]
    for case in (big, big, small, small, tiny, big, tiny):
        got, n = ctx.yolodec(case.data, case.layout, case.params, return_count=True)
        _check(got, n, case, "sequence")


def test_a_refused_call_leaves_the_context_usable(ctx):
    import mi355fx
    case = Y.group("random")[5]
    got, n = ctx.yolodec(case.data, case.layout, case.params, return_count=True)
    _check(got, n, case, "before")
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.yolodec(np.zeros((5, 10), np.float32), "V8", (0.5, 0.5, 0.5))
    assert e.value.status == mi355fx.ERR_INVALID_ARG
    with pytest.raises(mi355fx.Mi355Error) as e:
        ctx.yolodec(np.zeros((1030, 2), np.float32), "V8", (0.5, 0.5, 0.5))
    assert e.value.status == mi355fx.ERR_UNSUPPORTED
    d = ctx.alloc(4096)
    try:
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.yolodec_device(d, 6 * 10 * 4 - 4, 2, "X", 6, 10, [(0.5, 0.5, 0.5)] * 2)      # pitch smaller than the tensor
        assert e.value.status == mi355fx.ERR_INVALID_ARG
        with pytest.raises(mi355fx.Mi355Error) as e:
            ctx.yolodec_device(d + 2, 6 * 10 * 4, 1, "X", 6, 10, [(0.5, 0.5, 0.5)])          # misaligned
        assert e.value.status == mi355fx.ERR_INVALID_ARG
    finally:
        ctx.free(d)
    assert len(ctx.yolodec(np.zeros((6, 0), np.float32), "V8", (0.5, 0.5, 0.5))) == 0        # no candidates: no launch
    got, n = ctx.yolodec(case.data, case.layout, case.params, return_count=True)
    _check(got, n, case, "after")


@pytest.mark.parametrize("layout", ["V8", "X"])
def test_realistic_shape(ctx, layout):
    case = Y.realistic(layout)
    got, n = ctx.yolodec(case.data, case.layout, case.params, return_count=True)
    _check(got, n, case, "realistic")
    assert 0 < n < 130
