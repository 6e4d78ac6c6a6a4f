"""The YOLOX head decode contract without a device: the numpy restatement's known answers by hand, the class-tie
property of the many-to-one sigmoid, the discriminating power of the unfused case, the midpoint guard of every case, and the status
of every refusal of the entry points' shape checks (mi355_selftest_yolox_head_check)."""
import numpy as np
import pytest

import yolox_head_cases as H
import yolox_head_restate as R
from handdec_restate import near_tie

F32 = np.float32


def bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the restatement's known answers

def test_scalar_known_answers():
    assert bits(R.sigmoid32(0.0)) == bits(0.5)
    for s in (1, 7, 8, 32, 65536):
        assert bits(R.exp32(0.0) * F32(s)) == bits(float(s))
    assert bits(R.sigmoid32(20.0)) == bits(1.0) and bits(R.sigmoid32(-110.0)) == bits(0.0)
    assert bits(R.sigmoid32(17.0)) != bits(1.0) and R.sigmoid32(-100.0) > 0.0        # either side of the saturation points
    assert np.isposinf(R.exp32(88.8)) and np.isfinite(R.exp32(88.7))
    assert bits(R.sigmoid32(np.inf)) == bits(1.0) and bits(R.sigmoid32(-np.inf)) == bits(0.0)
    assert np.isnan(R.sigmoid32(np.nan)) and np.isnan(R.exp32(np.nan))


def test_grid_and_level_order_by_hand():
    head, rows = H.kat_head()
    t = head.tensor()
    assert t.shape == (14, 7)
    for cand, (cx, cy, w, h) in rows:
        assert [float(v) for v in t[cand, :4]] == [cx, cy, w, h], cand
        assert float(t[cand, 4]) == 1.0 and [float(v) for v in t[cand, 5:]] == [0.0, 0.5]
    got = head.expected()
    assert [int(d["candidate"]) for d in got] == [c for c, _ in rows]
    assert all(int(d["class_id"]) == 1 and float(d["confidence"]) == 0.5 for d in got)
    # xmin = cx - w / 2 ...; the ints add_od_mtd receives
    assert [(int(d["x"]), int(d["y"]), int(d["width"]), int(d["height"])) for d in got] == [(16, 6, 8, 8), (16, 28, 16, 16), (32, -8, 32, 32)]


def test_x_is_the_fast_index():
    reg = np.zeros((4, 2, 3), np.float32)
    lv = [(reg, np.zeros((1, 2, 3), np.float32), np.zeros((1, 2, 3), np.float32), 1)]
    t = R.tensor(lv)
    assert [tuple(r) for r in t[:, :2]] == [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]


# ---------------------------------------------------------------- the class is the last of equal SIGMOID maxima

def test_a_run_of_logits_with_one_sigmoid_yields_the_last_index():
    run = H.sigmoid_run()
    assert len(run) >= 4 and (np.diff(run) < 0).all() and len(set(bits(R.sigmoid32(run)).tolist())) == 1
    head, classes = H.tie_head()
    t = head.tensor()
    got = {int(d["candidate"]): int(d["class_id"]) for d in head.expected()}
    assert got == dict(enumerate(classes))
    # an argmax over the raw logits would have said otherwise for the run and for [20, 30, 25]
    raw = np.argmax(head.levels[0][2].reshape(head.C, -1), axis=0)
    assert raw[0] != classes[0] and raw[1] == 1 and classes[1] == 2
    assert classes[2] == head.C - 1 and float(t[2, 5:].max()) == 0.0


def test_the_unfused_case_has_discriminating_power():
    H.unfused_head()        # the builder asserts that one rounding would have differed for at least a quarter of the candidates


def test_objectness_drop_and_nonfinite_cases_by_hand():
    head, kept = H.objdrop_head()
    assert sorted(int(d["candidate"]) for d in head.expected()) == kept
    got = {int(d["candidate"]): d for d in H.nonfinite_head().expected()}
    assert len(got) == 8                                               # thresholds of 0 keep everything
    d = got[0]                                                         # w = inf: the box is (-inf, inf)
    assert np.isneginf(d["xmin"]) and np.isposinf(d["xmax"]) and int(d["x"]) == -2**31 and int(d["width"]) == 2**31 - 1
    assert np.isnan(got[1]["xmin"]) and int(got[1]["x"]) == 0 and int(got[1]["width"]) == 0
    assert int(got[2]["height"]) == 0
    for c in (4, 5):                                                   # a subnormal class or box confidence; -inf loses
        assert 0.0 < float(got[c]["confidence"]) < 1e-38 and int(got[c]["class_id"]) == 0
    assert int(got[7]["class_id"]) == 0 and float(got[7]["confidence"]) == 1.0             # sigmoid(17) < 1 = sigmoid(inf)


def test_near_tie_flags_no_value_of_any_case():
    heads = [H.shape_head(s, c) for s in H.LEVEL_SETS for c in H.CLASSES] + [H.kat_head()[0], H.tie_head()[0], H.unfused_head(), H.objdrop_head()[0],
                                                                              H.nonfinite_head(), H.trunc_head(3)] + H.batch_heads(3)
    for h in heads:
        assert not near_tie(R.deviation64(h.levels)).any(), h.name
    assert H.shape_head("boundary255", 2).A == 257


def test_input_tensor_by_hand():
    frame = np.array([1, 2, 3, 4, 5, 6, 0xEE, 7, 8, 9, 10, 11, 12, 0xEE], np.uint8)      # 2 x 2, stride 7
    t = R.input_tensor(frame, 7, 2, 2)
    assert t.tolist() == [[[1, 4], [7, 10]], [[2, 5], [8, 11]], [[3, 6], [9, 12]]]


# ---------------------------------------------------------------- the refusals

def _levels(n=3, h=4, w=5, C=3, stride=8, **over):
    """Valid device-form levels with made-up (never dereferenced) pointers."""
    out = []
    for l in range(n):
        hw = h * w
        lv = dict(reg=0x10000 * (l + 1), obj=0x10000 * (l + 1) + 0x4000, cls=0x10000 * (l + 1) + 0x8000, reg_pitch=16 * hw, obj_pitch=4 * hw,
                  cls_pitch=4 * C * hw, h=h, w=w, stride=stride, reserved=0)
        if l == n - 1:
            lv.update(over)
        out.append((lv["reg"], lv["obj"], lv["cls"], lv["reg_pitch"], lv["obj_pitch"], lv["cls_pitch"], lv["h"], lv["w"], lv["stride"], lv["reserved"]))
    return out


def _check(levels, n_tensors=2, C=3, out_pitch=None, n_levels=None):
    import mi355fx
    A = mi355fx.yolox_candidates(levels) if levels else 0
    return mi355fx.selftest_yolox_head_check(levels, n_tensors, C, A * (5 + C) * 4 if out_pitch is None else out_pitch, n_levels=n_levels)


def test_selftest_accepts_what_is_allowed(mi355lib):
    import mi355fx
    assert _check(_levels()) == mi355fx.OK
    assert _check(_levels(8, 1, 1)) == mi355fx.OK
    assert _check(_levels(1, 256, 256, C=1), C=1, n_tensors=1024) == mi355fx.OK          # A = 65536
    assert _check(_levels(1, 2, 2, C=1024), C=1024) == mi355fx.OK                        # 1029 fields
    assert _check(_levels(stride=65536)) == mi355fx.OK
    assert _check(_levels(reg_pitch=16 * 20 + 4, obj_pitch=4 * 20 + 8, cls_pitch=12 * 20 + 12), out_pitch=60 * 8 * 4 + 4) == mi355fx.OK
    # one allocation per level: obj = reg + 4 h w, cls = reg + 5 h w, equal pitches
    one = [(0x10000, 0x10000 + 16 * 20, 0x10000 + 20 * 20) + (4 * 8 * 20,) * 3 + (4, 5, 8, 0)]
    assert _check(one) == mi355fx.OK


@pytest.mark.parametrize("what", ["null_levels", "n_levels_0", "n_tensors_0", "classes_0", "h_0", "w_0", "stride_0", "reserved", "null_reg", "null_obj", "null_cls",
                                  "misaligned_reg", "misaligned_obj", "misaligned_cls", "reg_pitch_small", "obj_pitch_small", "cls_pitch_small",
                                  "reg_pitch_odd", "obj_pitch_odd", "cls_pitch_odd", "out_pitch_small", "out_pitch_odd"])
def test_selftest_invalid_arguments(mi355lib, what):
    import mi355fx
    rc = {
        "null_levels": lambda: _check(None, n_levels=3),
        "n_levels_0": lambda: _check(_levels(), n_levels=0),
        "n_tensors_0": lambda: _check(_levels(), n_tensors=0),
        "classes_0": lambda: _check(_levels(), C=0),
        "h_0": lambda: _check(_levels(h=0)),
        "w_0": lambda: _check(_levels(w=0)),
        "stride_0": lambda: _check(_levels(stride=0)),
        "reserved": lambda: _check(_levels(reserved=1)),
        "null_reg": lambda: _check(_levels(reg=0)),
        "null_obj": lambda: _check(_levels(obj=0)),
        "null_cls": lambda: _check(_levels(cls=0)),
        "misaligned_reg": lambda: _check(_levels(reg=0x10002)),
        "misaligned_obj": lambda: _check(_levels(obj=0x10001)),
        "misaligned_cls": lambda: _check(_levels(cls=0x10003)),
        "reg_pitch_small": lambda: _check(_levels(reg_pitch=16 * 20 - 4)),
        "obj_pitch_small": lambda: _check(_levels(obj_pitch=4 * 20 - 4)),
        "cls_pitch_small": lambda: _check(_levels(cls_pitch=12 * 20 - 4)),
        "reg_pitch_odd": lambda: _check(_levels(reg_pitch=16 * 20 + 2)),
        "obj_pitch_odd": lambda: _check(_levels(obj_pitch=4 * 20 + 1)),
        "cls_pitch_odd": lambda: _check(_levels(cls_pitch=12 * 20 + 3)),
        "out_pitch_small": lambda: _check(_levels(), out_pitch=60 * 8 * 4 - 4),
        "out_pitch_odd": lambda: _check(_levels(), out_pitch=60 * 8 * 4 + 2),
    }[what]()
    assert rc == mi355fx.ERR_INVALID_ARG


@pytest.mark.parametrize("what", ["levels_9", "fields_1030", "candidates_65537", "one_level_2_pow_32", "stride_65537", "tensors_1025"])
def test_selftest_unsupported_shapes(mi355lib, what):
    import mi355fx
    rc = {
        "levels_9": lambda: _check(_levels(8) + _levels(1)),
        "fields_1030": lambda: _check(_levels(1, 1, 1, C=1025), C=1025),
        "candidates_65537": lambda: _check(_levels(1, 256, 256, C=1) + _levels(1, 1, 1, C=1), C=1),
        "one_level_2_pow_32": lambda: _check(_levels(1, 65536, 65536, C=1), C=1, out_pitch=2**40),      # h * w in 64 bits
        "stride_65537": lambda: _check(_levels(stride=65537)),
        "tensors_1025": lambda: _check(_levels(), n_tensors=1025),
    }[what]()
    assert rc == mi355fx.ERR_UNSUPPORTED


# ---------------------------------------------------------------- numpy against C++

@pytest.fixture(scope="module")
def cpu_lib(tmp_path_factory):
    import ctypes as C
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++: the C++ restatement cannot be built")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("yolox_head_cpu") / "libyolox_head_cpu.so")
    subprocess.check_call([cxx, "-O3", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(root, "tools", "yolox_head_cpu.cpp"), "-o", so])
    L = C.CDLL(so)
    ptrs = [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint32)] * 3
    L.yolox_head_tensor_cpu.restype = L.yolox_head_dets_cpu.restype = C.c_int
    L.yolox_head_tensor_cpu.argtypes = ptrs + [C.c_int, C.c_uint32, C.c_void_p]
    L.yolox_head_dets_cpu.argtypes = ptrs + [C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


def cpu_level_args(levels):
    """The level arrays tools/yolox_head_cpu.cpp takes (the maps stay referenced by `levels`)."""
    import ctypes as C
    n = len(levels)
    reg, obj, cls = ((C.c_void_p * n)(*[lv[k].ctypes.data for lv in levels]) for k in range(3))
    h, w, s = ((C.c_uint32 * n)(*v) for v in ([lv[0].shape[1] for lv in levels], [lv[0].shape[2] for lv in levels], [lv[3] for lv in levels]))
    return [reg, obj, cls, h, w, s, n]


def test_cpp_restatement_equals_numpy(cpu_lib):
    import ctypes as C
    heads = [H.shape_head(s, c) for s in H.LEVEL_SETS for c in (1, 80)] + [H.kat_head()[0], H.tie_head()[0], H.unfused_head(), H.nonfinite_head(), H.trunc_head(7)]
    for head in heads:
        args = cpu_level_args(head.levels)
        t = np.zeros((head.A, 5 + head.C), np.float32)
        assert cpu_lib.yolox_head_tensor_cpu(*args, head.C, t.ctypes.data) == 0
        assert R.same_tensor(t, head.tensor()), head.name
        cap = head.A if head.max_dets is None else head.max_dets
        dets, n = np.zeros(max(cap, 1), R.DET), C.c_uint32(0)
        assert cpu_lib.yolox_head_dets_cpu(*args, head.C, *head.params, t.ctypes.data, dets.ctypes.data, cap, C.byref(n)) == 0
        want = head.expected()
        assert n.value == len(want) and R.same_records(dets[:min(n.value, cap)], want[:cap]), head.name
