"""yolov8tensordec2 / yoloxtensordec without a GPU: the hand-written known answers against the numpy restatement
(tests/yolodec_restate.py), the numpy restatement against the C++ one (tools/yolodec_cpu.cpp) on every case of
tests/yolodec_cases.py with all fields compared as bits, and the argument checks of the new entry points that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import yolodec_cases as Y
import yolodec_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- known answers

def test_iou_of_the_kat_boxes_is_exactly_one_half():
    one = np.float32
    got = R.iou_kept(np.array([0], one), np.array([0], one), np.array([9], one), np.array([9], one), one(0), one(0), one(9), one(4))
    assert got.dtype == np.float32 and got.view(np.uint32)[0] == np.float32(0.5).view(np.uint32)
    assert np.float32(Y.IOU_HALF_BELOW) < np.float32(0.5)


@pytest.mark.parametrize("k", range(6))
def test_known_answers(k):
    case, rows, confs = Y.kats()[k]
    got = case.expected()
    assert [(int(d["x"]), int(d["y"]), int(d["width"]), int(d["height"]), int(d["class_id"]), int(d["candidate"])) for d in got] == rows
    assert [d["confidence"].view(np.uint32) for d in got] == [np.float32(c).view(np.uint32) for c in confs]
    assert not got["reserved"].any()


def test_argmax_rule():
    for case, classes in Y.argmax_cases():
        got = case.expected()
        by_cand = {int(d["candidate"]): int(d["class_id"]) for d in got}
        assert [by_cand[c] for c in range(case.N)] == classes, case.name     # every candidate is kept


def test_positive_nan_sorts_first_in_its_class_and_negative_nan_loses():
    cases = {c.name: c for c, _ in Y.argmax_cases()}
    got = cases["nan_pos_V8"].expected()
    assert [int(c) for c in got["candidate"]] == [0, 1] and got["confidence"].view(np.uint32)[0] == Y.QNAN_POS
    got = cases["nan_neg_V8"].expected()
    assert not np.isnan(got["confidence"]).any()


def test_total_key_is_total_cmp():
    u = np.array([0xFFFFFFFF, Y.QNAN_NEG, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0, 1, 0x3F800000, 0x7F800000, 0x7F800001, Y.QNAN_POS],
                 np.uint32)
    k = R.total_key(u.view(np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all()


def test_ties_follow_the_candidate_index():
    plain, permuted = Y.tie_cases()
    a, b = plain.expected(), permuted.expected()
    # boxes 4 apart, 10 wide (11 with the + 1): neighbours overlap 77 / 165 > 0.3, next-but-one 33 / 209 < 0.3
    assert [int(c) for c in a["candidate"]] == [0, 2, 4]
    assert int(b["candidate"][0]) == 0 and (np.diff(b["candidate"].astype(np.int64)) > 0).all()
    # the permuted tensor's answer is another set of BOXES: the order decides
    assert sorted(Y.TIE_PERM[int(c)] for c in b["candidate"]) == [0, 3, 5]


def test_casts():
    for layout in ("V8", "X"):
        got = Y.cast_case(layout).expected()
        d = {int(r["candidate"]): r for r in got}
        assert sorted(d) == [0, 1, 2, 3, 4, 5]                   # 6 is dropped by 5; the NaN box drops nothing and stays
        i32 = np.iinfo(np.int32)
        assert (d[0]["x"], d[0]["y"]) == (i32.max, i32.max) and (d[1]["x"], d[1]["y"]) == (i32.min, i32.min)
        assert (d[2]["x"], d[2]["y"], d[2]["width"], d[2]["height"]) == (0, 0, 10, 19)
        assert (d[3]["width"], d[3]["height"]) == (0, 0)
        assert np.isnan(d[4]["xmin"]) and (d[4]["x"], d[4]["width"], d[4]["y"], d[4]["height"]) == (0, 0, 295, 10)
        assert int(got["candidate"][0]) == 4                     # the most confident box: first in the class


def test_survivor_counts():
    for c in Y.group("survivors"):
        n = len(c.expected())
        if c.name.startswith("none"):
            assert n == 0
        elif c.name.startswith("one"):
            assert n == 1 and int(c.expected()["candidate"][0]) == 123
        else:
            assert 0 < n < c.N                                  # everything survives the thresholds, NMS drops some
    for c in Y.group("sort_switch"):
        n = len(c.expected())
        assert c.N // 8 < n < c.N, (c.name, n)                  # NMS both keeps and drops


def test_realistic_tensors_have_about_one_percent_survivors():
    for layout in ("V8", "X"):
        c = Y.realistic(layout)
        n = len(R.candidates(c.data, layout, c.params[0], c.params[1])[0])
        assert 50 <= n <= 130, (layout, n)
        assert 0 < len(c.expected()) < n


# ---------------------------------------------------------------- numpy against C++

@pytest.fixture(scope="module")
def cpu_lib(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++: the C++ restatement cannot be built")
    so = str(tmp_path_factory.mktemp("yolodec_cpu") / "libyolodec_cpu.so")
    subprocess.check_call([cxx, "-O3", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tools", "yolodec_cpu.cpp"), "-o", so])
    L = C.CDLL(so)
    L.yolodec_cpu.restype = C.c_int
    L.yolodec_cpu.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


def _cpu(L, case, cap):
    dets = np.zeros(max(cap, 1), R.DET)
    n = C.c_uint32(0)
    rc = L.yolodec_cpu(case.data.ctypes.data, 0 if case.layout == "V8" else 1, case.F, case.N, *case.params, dets.ctypes.data, cap, C.byref(n))
    assert rc == 0
    return dets[:min(n.value, cap)], n.value


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", Y.GROUPS)
def test_cpp_restatement_equals_numpy_restatement(cpu_lib, name):
    for case in Y.group(name):
        want = case.expected()
        cap = case.N if case.max_dets is None else case.max_dets
        got, n = _cpu(cpu_lib, case, cap)
        assert n == len(want), case.name
        assert _same_bits(got, want[:cap]), case.name


def test_cpp_restatement_on_the_realistic_shapes(cpu_lib):
    for layout in ("V8", "X"):
        case = Y.realistic(layout)
        got, n = _cpu(cpu_lib, case, case.N)
        assert n == len(case.expected()) and _same_bits(got, case.expected())


# ---------------------------------------------------------------- ABI surface and the checks that need no device

NEW_SYMBOLS = ("mi355_yolodec_tensor", "mi355_yolodec_tensors_device", "mi355_selftest_yolodec_check")


def test_library_exports_the_entry_points(mi355lib):
    import mi355fx
    hdr = open(mi355fx.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr and hasattr(mi355lib, name) and getattr(mi355lib, name).argtypes is not None, name
    assert mi355lib.mi355_abi_version() == 1


def test_record_and_settings_match_the_header_layout():
    import mi355fx
    assert mi355fx.YOLO_DET.itemsize == 48 and mi355fx.YOLO_DET == R.DET
    assert [mi355fx.YOLO_DET.fields[n][1] for n in ("xmin", "x", "class_id", "confidence", "candidate", "reserved")] == [0, 16, 32, 36, 40, 44]
    assert C.sizeof(mi355fx.YoloParams) == 12 and mi355fx.YoloParams.iou_threshold.offset == 8
    assert mi355fx.YOLO_LAYOUT == {"V8": 0, "X": 1}


def test_shape_checks(mi355lib):
    import mi355fx
    chk = mi355lib.mi355_selftest_yolodec_check
    ok = lambda F, N, T=1, layout=0, pitch=None: chk(F * N * 4 if pitch is None else pitch, T, layout, F, N)
    assert ok(6, 0) == 0 and ok(6, 1) == 0 and ok(1029, 65536, 1024) == 0 and ok(85, 8400, 256, 1) == 0
    for F in (0, 4, 5):
        assert ok(F, 100) == mi355fx.ERR_INVALID_ARG                       # find_yolo_tensor_meta refuses fewer than 6 fields
        assert ok(F, 65537) == mi355fx.ERR_INVALID_ARG
    assert ok(1030, 100) == mi355fx.ERR_UNSUPPORTED
    assert ok(6, 65537) == mi355fx.ERR_UNSUPPORTED
    assert ok(6, 100, 1025) == mi355fx.ERR_UNSUPPORTED
    assert ok(6, 100, 0) == mi355fx.ERR_INVALID_ARG and ok(6, 100, -1) == mi355fx.ERR_INVALID_ARG
    assert ok(6, 100, 1, 2) == mi355fx.ERR_INVALID_ARG and ok(6, 100, 1, -1) == mi355fx.ERR_INVALID_ARG
    assert ok(6, 100, 4, 0, 2400 - 4) == mi355fx.ERR_INVALID_ARG             # pitch smaller than the tensor
    assert ok(6, 100, 4, 0, 2402) == mi355fx.ERR_INVALID_ARG                 # pitch no multiple of 4
    assert ok(6, 100, 4, 0, 2404) == 0


def test_null_context_is_refused(mi355lib):
    import mi355fx
    p = mi355fx.YoloParams(0.5, 0.5, 0.5)
    n = C.c_uint32(7)
    assert mi355lib.mi355_yolodec_tensor(None, None, 0, 6, 0, C.byref(p), None, 0, C.byref(n)) == mi355fx.ERR_INVALID_ARG
    assert mi355lib.mi355_yolodec_tensors_device(None, None, 0, 1, 0, 6, 0, C.byref(p), None, 0, C.byref(n)) == mi355fx.ERR_INVALID_ARG
    assert n.value == 7
