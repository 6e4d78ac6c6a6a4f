"""The infer side of a decoder launch set's layout, without a device (mi355_selftest_yolox_infer_set_plan): which
infer members of a set share a forward - classes by (net, H, W), numbered by first appearance in submit order, their frames in submit
order - and where each member's blocks stand in the one conversion launch. The queue plans its sets with the same function; the
decode side of an infer job is a head job's (tests/test_group_yolox_head_cpu.py) and is not restated here."""
import pytest

import mi355fx

V8, X, HEAD, INFER = 0, 1, mi355fx.YOLO_X_HEAD, mi355fx.YOLO_X_INFER
OK, INVALID, UNSUPPORTED = 0, mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED
SET_MAX = 32


def restate(kinds, keys, hs, ws):
    """the table of the issue, in a few lines"""
    classes, class_of, frame_in, first, blocks, frames = [], [], [], [], [], []
    at = 0
    for kind, key, h, w in zip(kinds, keys, hs, ws):
        first.append(at)
        if kind != INFER:
            class_of.append(-1)
            frame_in.append(None)           # not read
            blocks.append(0)
            continue
        if (key, h, w) not in classes:
            classes.append((key, h, w))
            frames.append(0)
        c = classes.index((key, h, w))
        class_of.append(c)
        frame_in.append(frames[c])
        frames[c] += 1
        blocks.append(-(-((w // 4) * h) // 256))
        at += blocks[-1]
    return class_of, frame_in, first, blocks, frames, [len(classes), sum(frames), at]


def check(kinds, keys, hs, ws):
    rc, class_of, frame_in, first, blocks, frames, totals = mi355fx.selftest_yolox_infer_set_plan(kinds, keys, hs, ws)
    want = restate(kinds, keys, hs, ws)
    assert rc == OK
    assert class_of == want[0] and first == want[2] and blocks == want[3] and frames == want[4] and totals == want[5]
    assert all(w is None or g == w for g, w in zip(frame_in, want[1]))
    return class_of, frame_in, first, blocks, frames, totals


def test_constants():
    assert (V8, X, HEAD, INFER) == (0, 1, 2, 3) and mi355fx.YOLO_LAYOUT == {"V8": 0, "X": 1}


def test_mixed_kinds_and_classes_by_first_appearance():
    # a V8 tensor, net 7 at 64 x 96, a head, net 9 at 64 x 96, net 7 at 32 x 32, an X tensor, net 7 at 64 x 96 again, net 9 again
    kinds = [V8, INFER, HEAD, INFER, INFER, X, INFER, INFER]
    keys = [0, 7, 0, 9, 7, 0, 7, 9]
    hs = [0, 64, 0, 64, 32, 0, 64, 64]
    ws = [0, 96, 0, 96, 32, 0, 96, 96]
    class_of, frame_in, first, blocks, frames, totals = check(kinds, keys, hs, ws)
    assert class_of == [-1, 0, -1, 1, 2, -1, 0, 1]
    assert [frame_in[j] for j in (1, 3, 4, 6, 7)] == [0, 0, 0, 1, 1]
    assert blocks == [0, 6, 0, 6, 1, 0, 6, 6] and first == [0, 0, 6, 6, 12, 13, 13, 19]
    assert frames == [2, 2, 1] and totals == [3, 5, 25]


def test_one_net_at_two_sizes_is_two_classes():
    _, _, _, _, frames, totals = check([INFER] * 4, [5, 5, 5, 5], [32, 64, 32, 64], [32, 96, 32, 96])
    assert frames == [2, 2] and totals[:2] == [2, 4]
    # ... and the transposed size is a class of its own
    assert check([INFER] * 2, [5, 5], [64, 96], [96, 64])[5][0] == 2


def test_two_nets_at_one_size_are_two_classes():
    class_of, frame_in, _, _, frames, _ = check([INFER] * 3, [11, 12, 11], [64] * 3, [96] * 3)
    assert class_of == [0, 1, 0] and frame_in == [0, 0, 1] and frames == [2, 1]
    # the keys are whole 64-bit numbers
    assert check([INFER] * 2, [1 << 40, (1 << 40) + 1], [32] * 2, [32] * 2)[0] == [0, 1]


def test_a_full_set_of_one_class():
    class_of, frame_in, first, blocks, frames, totals = check([INFER] * SET_MAX, [3] * SET_MAX, [640] * SET_MAX, [640] * SET_MAX)
    assert class_of == [0] * SET_MAX and frame_in == list(range(SET_MAX)) and frames == [SET_MAX]
    assert blocks == [400] * SET_MAX and first == [400 * j for j in range(SET_MAX)] and totals == [1, SET_MAX, 400 * SET_MAX]


def test_sizes_at_the_limits():
    assert check([INFER, INFER], [1, 1], [2048, 32], [2048, 2048])[3] == [4096, 64]


def test_no_infer_job_reads_nothing_of_the_three():
    # a tensor or head job's key and size are not read: sizes no net would take are fine there
    rc, class_of, _, first, blocks, frames, totals = mi355fx.selftest_yolox_infer_set_plan([V8, X, HEAD], [1, 2, 3], [33, 0, 4096], [5, 0, 7])
    assert rc == OK and class_of == [-1, -1, -1] and first == [0, 0, 0] and blocks == [0, 0, 0] and frames == [] and totals == [0, 0, 0]


def test_empty_set():
    rc, class_of, _, _, _, frames, totals = mi355fx.selftest_yolox_infer_set_plan([], [], [], [])
    assert rc == OK and class_of == [] and frames == [] and totals == [0, 0, 0]
    # no array is read or written for no job
    L = mi355fx.load_library()
    import ctypes as C
    totals = (C.c_uint64 * 3)(9, 9, 9)
    assert L.mi355_selftest_yolox_infer_set_plan(0, None, None, None, None, None, None, None, None, None, totals) == OK and list(totals) == [0, 0, 0]


def test_refusals():
    import ctypes as C
    L = mi355fx.load_library()
    one = dict(kinds=[INFER], net_keys=[1], heights=[32], widths=[32])
    assert mi355fx.selftest_yolox_infer_set_plan(**one)[0] == OK
    for name in ("kind", "net_key", "height", "width", "class_of", "frame_in_class", "conv_first_block", "conv_blocks", "class_frames", "totals"):
        assert mi355fx.selftest_yolox_infer_set_plan(null=(name,), **one)[0] == INVALID, name
    # the arrays are wanted for any job, an infer one or not
    assert mi355fx.selftest_yolox_infer_set_plan([V8], [0], [0], [0], null=("class_frames",))[0] == INVALID
    assert mi355fx.selftest_yolox_infer_set_plan([], [], [], [], null=("totals",))[0] == INVALID
    n = SET_MAX + 1
    assert mi355fx.selftest_yolox_infer_set_plan([INFER] * n, [1] * n, [32] * n, [32] * n)[0] == INVALID
    totals = (C.c_uint64 * 3)()
    assert L.mi355_selftest_yolox_infer_set_plan(-1, None, None, None, None, None, None, None, None, None, totals) == INVALID
    for kind in (-1, 4, 100):
        assert mi355fx.selftest_yolox_infer_set_plan([INFER, kind], [1, 1], [32, 32], [32, 32])[0] == INVALID, kind


@pytest.mark.parametrize("h,w,status", [(33, 32, INVALID), (32, 33, INVALID), (0, 32, INVALID), (32, 0, INVALID), (48, 64, INVALID), (2080, 32, UNSUPPORTED),
                                        (32, 2080, UNSUPPORTED), (2048, 2048, OK)])
def test_a_bad_size_has_the_nets_status(h, w, status):
    assert mi355fx.selftest_yolox_infer_set_plan([INFER], [1], [h], [w])[0] == status
    assert mi355fx.selftest_yolox_infer_set_plan([X, INFER], [1, 1], [0, h], [0, w])[0] == status      # behind another job too
    # the same status the net's own plan gives the size
    cfg = mi355fx.yolox_net_config(0.33, 0.25, True, 1)
    assert mi355fx.selftest_yolox_net_plan(cfg, 1, h, w)[1].size_status == status
