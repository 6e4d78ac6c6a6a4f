"""handdetectiontensordec / handlandmarktensordec on the GPU: the four mi355_handdec_* entry points against the numpy restatement
(tests/handdec_restate.py) on every case of tests/handdec_cases.py - every record field bit-equal (f32 fields with
NaN == NaN), the counts equal - and the batch, pitch, repeat and refusal behaviour of the entry points."""
import numpy as np
import pytest

import handdec_cases as H
import handdec_restate as R

pytestmark = pytest.mark.gpu

POISON = np.float32(7e30)   # in the padding between tensors: as a score it would survive any threshold


def _why(got, want):
    """the f64 values a disagreement is judged by are the restatement's; show both records"""
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


def _upload(ctx, arrays, pad_floats=0):
    """arrays of one size side by side at a pitch of size + pad_floats floats, poison in the padding -> (device pointer, pitch bytes)"""
    n = arrays[0].size
    pitch = n + pad_floats
    buf = np.full(max(pitch * len(arrays), 4), POISON, np.float32)
    for k, a in enumerate(arrays):
        buf[k * pitch:k * pitch + n] = a.reshape(-1)
    d = ctx.alloc(buf.nbytes)
    ctx.h2d(d, buf)
    return d, pitch * 4


def _palm_device(ctx, tensors, params, pad_floats=0):
    d, pitch = _upload(ctx, tensors, pad_floats)
    try:
        return ctx.handdec_palm_device(d, pitch, len(tensors), tensors[0].shape[0], [H.flat_params(p) for p in params])
    finally:
        ctx.free(d)


def _landmarks_device(ctx, tensors, scores, params, pad_floats=0):
    """scores: None or one vector per tensor, all of one length"""
    Hn, D = tensors[0].shape[0], tensors[0].shape[1] // 21
    d, pitch = _upload(ctx, tensors, pad_floats)
    ds, spitch, ns = None, 0, 0
    try:
        if scores is not None and len(scores[0]):
            ds, spitch = _upload(ctx, scores, pad_floats)
            ns = len(scores[0])
        return ctx.handdec_landmarks_device(d, pitch, len(tensors), Hn, D, [H.flat_params(p) for p in params], ds, spitch, ns)
    finally:
        ctx.free(d)
        if ds is not None:
            ctx.free(ds)


PALM_GROUPS = {"random": H.palm_random, "written": H.palm_written, "iou_pair": lambda: [c for c, _ in H.palm_iou_pair()]}
LANDMARK_GROUPS = {"random": H.landmarks_random, "written": H.landmarks_written, "iou_pair": lambda: [c for c, _ in H.landmarks_iou_pair()]}


@pytest.mark.parametrize("name", sorted(PALM_GROUPS))
def test_palm_cases_match_the_restatement(ctx, name):
    for case in PALM_GROUPS[name]():
        _check_palm(ctx.handdec_palm(case.data, H.flat_params(case.params)), case, "host tensor")
        if case.N:
            _check_palm(_palm_device(ctx, [case.data], [case.params])[0], case, "device tensor")


@pytest.mark.parametrize("name", sorted(LANDMARK_GROUPS))
def test_landmark_cases_match_the_restatement(ctx, name):
    for case in LANDMARK_GROUPS[name]():
        _check_landmarks(ctx.handdec_landmarks(case.data, H.flat_params(case.params), case.scores), case, "host tensor")
        if case.H:
            sc = None if case.scores is None else [case.scores]
            _check_landmarks(_landmarks_device(ctx, [case.data], sc, [case.params])[0], case, "device tensor")


def test_palm_known_answer_by_hand(ctx):
    got = ctx.handdec_palm(np.array([H.palm_row(0.9, 0.5, 0.6, 0.2)], np.float32), (0.5, 0.3, 2, 192, 192))
    assert len(got) == 1 and (int(got["x"][0]), int(got["y"][0]), int(got["width"][0]), int(got["height"][0])) == (40, 40, 112, 112)
    assert got["rotation"][0] == 0 and got["rotation_od"][0] == -R.FRAC_PI_2 and got["has_od"][0] == 1 and got["confidence"][0] == np.float32(0.9)


def _palm_settings(k):
    rng = np.random.default_rng(40 + k)
    return (float(rng.uniform(0.0, 0.8)), float(rng.uniform(0.0, 0.6)), 1 + k % 8, H.FRAMES[k % 3])


def _landmark_settings(k):
    rng = np.random.default_rng(60 + k)
    return (float(rng.uniform(0.2, 0.8)), float(rng.uniform(-0.1, 0.6)), 1 + k % 10, H.FRAMES[1 + k % 2])


@pytest.mark.parametrize("n_tensors", [1, 3, 33])
def test_palm_batches_with_their_own_params_equal_lone_calls(ctx, n_tensors):
    tensors = [H.palm_synth(300 + k, 333) for k in range(n_tensors)]
    params = [_palm_settings(k) for k in range(n_tensors)]
    got = _palm_device(ctx, tensors, params, pad_floats=0 if n_tensors == 3 else 37)     # 37 floats: the later tensors are not 16-byte aligned
    for k in range(n_tensors):
        want = R.palm_decode(tensors[k], *params[k])
        lone = ctx.handdec_palm(tensors[k], H.flat_params(params[k]))
        assert R.same_records(got[k], want) and R.same_records(lone, want), k
    assert len({len(g) for g in got}) > 1 or n_tensors == 1


@pytest.mark.parametrize("n_tensors", [1, 3, 33])
def test_landmark_batches_with_their_own_params_equal_lone_calls(ctx, n_tensors):
    rngs = [np.random.default_rng(700 + k) for k in range(n_tensors)]
    tensors = [H.hand_synth(r, 23, 3) for r in rngs]
    scores = [r.uniform(0, 1, 17).astype(np.float32) for r in rngs]
    params = [_landmark_settings(k) for k in range(n_tensors)]
    got = _landmarks_device(ctx, tensors, scores, params, pad_floats=0 if n_tensors == 3 else 5)
    for k in range(n_tensors):
        want = R.landmarks_decode(tensors[k], scores[k], *params[k])
        lone = ctx.handdec_landmarks(tensors[k], H.flat_params(params[k]), scores[k])
        for a, b, c in zip(got[k], lone, want):
            assert R.same_records(a, c) and R.same_records(b, c), k
    assert len({len(g[0]) for g in got}) > 1 or n_tensors == 1


def test_palm_batch_with_empty_and_full_tensors(ctx):
    tensors = [H.palm_synth(500 + k, 700) for k in range(4)]
    params = [(0.3, 0.08, 2, None), (5.0, 0.08, 8, None), (-1.0, 1.0, 8, (640, 360)), (0.3, 0.08, 8, (192, 192))]
    got = _palm_device(ctx, tensors, params, pad_floats=3)
    assert len(got[1]) == 0 and len(got[2]) == 8 and len(got[0]) == 2
    for k in range(4):
        assert R.same_records(got[k], R.palm_decode(tensors[k], *params[k])), k


def test_big_then_small_on_one_context(ctx):
    big = [c for c in H.palm_random() if c.name == "random_N4096_kNone"][0]
    small = [c for c in H.palm_random() if c.name == "random_N63_kNone"][0]
    lbig = [c for c in H.landmarks_random() if c.name == "random_H1024_D4_absent"][0]
    lsmall = [c for c in H.landmarks_random() if c.name == "random_H2_D2_full"][0]
    for case in (big, lbig, big, small, lsmall, lsmall, small, lbig, big):
        if isinstance(case, H.PalmCase):
            _check_palm(ctx.handdec_palm(case.data, H.flat_params(case.params)), case, "sequence")
        else:
            _check_landmarks(ctx.handdec_landmarks(case.data, H.flat_params(case.params), case.scores), case, "sequence")


def test_a_refused_call_leaves_the_context_usable(ctx):
    import mi355fx
    pcase = [c for c in H.palm_random() if c.name == "random_N255_k33"][0]
    lcase = [c for c in H.landmarks_random() if c.name == "random_H11_D3_short"][0]
    _check_palm(ctx.handdec_palm(pcase.data, H.flat_params(pcase.params)), pcase, "before")
    _check_landmarks(ctx.handdec_landmarks(lcase.data, H.flat_params(lcase.params), lcase.scores), lcase, "before")

    def refused(status, fn, *args):
        with pytest.raises(mi355fx.Mi355Error) as e:
            fn(*args)
        assert e.value.status == status

    INV, UNS = mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED
    refused(UNS, ctx.handdec_palm, np.zeros((4097, 8), np.float32), (0.5, 0.3, 2))
    refused(INV, ctx.handdec_palm, pcase.data, (0.5, 0.3, 9))
    refused(INV, ctx.handdec_palm, pcase.data, (0.5, 0.3, 0))
    refused(INV, ctx.handdec_palm, pcase.data, (0.5, 0.3, 2, 192, 0))
    refused(UNS, ctx.handdec_landmarks, np.zeros((1025, 42), np.float32), (0.5, 0.3, 2, 640, 360))
    refused(INV, ctx.handdec_landmarks, np.zeros((3, 21), np.float32), (0.5, 0.3, 2, 640, 360))
    refused(UNS, ctx.handdec_landmarks, np.zeros((3, 21 * 17), np.float32), (0.5, 0.3, 2, 640, 360))
    refused(INV, ctx.handdec_landmarks, lcase.data, (0.5, 0.3, 11, 640, 360))
    d = ctx.alloc(4096)
    try:
        refused(INV, ctx.handdec_palm_device, d, 10 * 32 - 4, 2, 10, [(0.5, 0.3, 2)] * 2)            # pitch smaller than the tensor
        refused(INV, ctx.handdec_palm_device, d + 2, 10 * 32, 1, 10, [(0.5, 0.3, 2)])                # misaligned
        refused(INV, ctx.handdec_palm_device, d, 10 * 32, 2, 10, [(0.5, 0.3, 2), (0.5, 0.3, 9)])     # the second tensor's max_hands
        refused(INV, ctx.handdec_landmarks_device, d, 2 * 63 * 4, 1, 2, 3, [(0.5, 0.3, 2)], d + 1024, 6, 2)   # score pitch no multiple of 4
        refused(INV, ctx.handdec_landmarks_device, d, 2 * 63 * 4, 1, 2, 3, [(0.5, 0.3, 2)], d + 1026, 8, 2)   # misaligned scores
    finally:
        ctx.free(d)
    assert len(ctx.handdec_palm(np.zeros((0, 8), np.float32), (0.5, 0.3, 2))) == 0                   # no rows: no launch
    assert len(ctx.handdec_landmarks(np.zeros((0, 63), np.float32), (0.5, 0.3, 2))[0]) == 0
    _check_palm(ctx.handdec_palm(pcase.data, H.flat_params(pcase.params)), pcase, "after")
    _check_landmarks(ctx.handdec_landmarks(lcase.data, H.flat_params(lcase.params), lcase.scores), lcase, "after")
