"""handdetectiontensordec / handlandmarktensordec without a GPU: the reference's own unit-test numbers (tests/golden/
handdec_reference_kats.json) and hand-written known answers against the numpy restatement (tests/handdec_restate.py), the numpy
restatement against the C++ one (tools/handdec_cpu.cpp) on every case of tests/handdec_cases.py with all fields compared as bits, the
rounding-midpoint guard of deviation a, and the argument checks of the new entry points that need no device."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import handdec_cases as H
import handdec_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---------------------------------------------------------------- known answers

@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "handdec_reference_kats.json")))


def test_reference_oriented_od_known_answers(golden):
    assert len(golden["oriented_od_params"]) == 5
    for k in golden["oriented_od_params"]:
        got = R.oriented_od([F32(v) for v in k["bbox"]], F32(k["rotation"]), tuple(k["frame"]))
        assert (None if got is None else list(got[:4])) == k["expect"], k["name"]
    m = golden["rotation_mapping"]
    got = R.oriented_od([F32(v) for v in m["bbox"]], F32(m["rotation"]), tuple(m["frame"]))
    assert abs(float(got[4]) + np.pi / 2) < m["expect_rotation_od_plus_frac_pi_2_abs_below"]


def test_reference_rotation_known_answers(golden):
    for k in golden["rotation_checks"]:
        if k["name"] == "angle_from_vector":
            got = float(F32(R.atan2_64(F32(k["dy"]), F32(k["dx"]))))
            assert abs(got - k["expect"]) < k["abs_below"]
        elif k["name"] == "palm_rotation_from_keypoints":
            (x0, y0), (x2, y2) = np.float32(k["kp0"]), np.float32(k["kp2"])      # (a row with this span is no valid palm: rule 2 alone)
            rot = R.FRAC_PI_2 + F32(R.atan2_64(y2 - y0, x2 - x0))
            assert abs(float(rot) - k["expect"]) < k["abs_below"]
        else:
            pts = np.zeros((1, 21, k["kps_dim"]), np.float32)
            pts[0, 0, :2], pts[0, 9, :2] = k["wrist"], k["middle_base"]
            pts[0, 5, :2] = (3.0, 4.0)                                 # a box: the all-zero hand of the reference's test has none
            dets, _ = R.landmarks_decode(pts.reshape(1, -1), None, 0.5, 0.2, 2, (100, 100))
            assert len(dets) == 1 and dets["has_od"][0] == 1 and abs(float(dets["rotation_od"][0]) - k["expect_rotation_od"]) < k["abs_below"]


def test_palm_known_answers_by_hand():
    # rotation 0 (kp2 straight above kp0): center = (0.5, 0.6 - 0.1), rr = 0.58 -> 111.36 px of a 192 frame
    row = np.array([H.palm_row(0.9, 0.5, 0.6, 0.2)], np.float32)
    d = R.palm_decode(row, 0.5, 0.3, 2, (192, 192))
    assert len(d) == 1 and d["rotation"][0] == 0 and d["index"][0] == 0 and d["confidence"][0] == F32(0.9) and d["has_od"][0] == 1
    assert (int(d["x"][0]), int(d["y"][0]), int(d["width"][0]), int(d["height"][0])) == (40, 40, 112, 112)
    assert d["rotation_od"][0] == -R.FRAC_PI_2
    # 640 x 360: rr scales by max(w, h) = 640
    d = R.palm_decode(row, 0.5, 0.3, 2, (640, 360))
    assert abs(float(d["xmax"][0] - d["xmin"][0]) - 0.58 * 640) < 1e-3 and abs(float(d["ymax"][0] - d["ymin"][0]) - 0.58 * 640) < 1e-3
    # no frame: the normalised box, nothing dropped by the frame test
    d = R.palm_decode(row, 0.5, 0.3, 2, None)
    assert abs(float(d["xmin"][0]) - 0.21) < 1e-6 and (int(d["x"][0]), int(d["width"][0])) == (0, 1)


def test_palm_written_cases_say_what_they_are_meant_to():
    c = {k.name: k for k in H.palm_written()}
    assert len(c["all_dropped"].expected()) == 0
    for mh in (1, 8):
        for name in ("all_valid_iou1_max%d", "all_valid_iou_above1_max%d"):
            got = c[name % mh].expected()
            assert [int(i) for i in got["index"]] == list(range(99, 99 - mh, -1))        # only max_hands stops the walk
    assert [int(i) for i in c["stacked_iou0"].expected()["index"]] == [99]
    assert [int(i) for i in c["equal_scores"].expected()["index"]] == list(range(8))     # equal keys: ascending row index
    got = c["equal_scores_interleaved"].expected()                                       # 0.9 rows first, then 0.75 rows, each by row index
    assert (np.diff(R.total_key(got["confidence"]).astype(np.int64)) <= 0).all() and got["confidence"][0] == F32(0.9)
    same = got["confidence"][:-1] == got["confidence"][1:]
    assert (np.diff(got["index"].astype(np.int64))[same] > 0).all() and same.any()
    got = c["nan_scores"].expected()
    assert got["confidence"].view(np.uint32)[0] == H.QNAN_POS and np.isinf(got["confidence"][1]) and got["confidence"].view(np.uint32)[-1] == H.QNAN_NEG
    assert len(c["nan_threshold"].expected()) == 8                                      # a NaN threshold drops nothing, a NaN IoU threshold neither
    assert sorted(int(i) for i in c["bad_sizes"].expected()["index"]) == [0, 6, 7]
    assert sorted(int(i) for i in c["non_finite_fields"].expected()["index"]) == [0, 7]
    facts = H.centre_edge_facts()
    assert facts[0] == 0 and facts[1] == 1 and facts[2] < 0 and facts[3] == 1
    idx = sorted(int(i) for i in c["centre_on_the_edges"].expected()["index"])
    assert 0 in idx and 2 not in idx and 4 in idx and 5 in idx                          # centre exactly 0 with exactly half the box visible stays
    for case, n in H.palm_iou_pair():
        assert len(case.expected()) == n, case.name                                      # strict >


def test_landmark_written_cases_say_what_they_are_meant_to():
    c = {k.name: k for k in H.landmarks_written()}
    for D in (2, 3, 4):
        dets, kps = c["special_D%d_absent" % D].expected()
        assert [int(i) for i in dets["index"]] == [2, 3, 4, 5]                           # 0 and 1 have no box; equal confidences: by hand index
        assert np.isnan(dets["rotation"][0]) and np.isnan(dets["rotation_od"][0]) and dets["has_od"][0] == 1
        assert dets["rotation"][1] == 0                                                  # atan2(-inf, 1) = -pi / 2
        assert [int(n) for n in kps["count"]] == [20, 20, 18, 21]
        if D == 2:
            assert (kps["visibilities"] == R.KP_UNKNOWN).all() and (kps["confidences"][:, :18] == 1).all()   # the hand's confidence
        else:
            assert [int(v) for v in kps["visibilities"][3][:7]] == [2, 1, 2, 2, 1, 2, 1]  # 0.5 occluded, just above visible, NaN occluded
        dets, _ = c["special_D%d_short" % D].expected()
        assert [int(i) for i in dets["index"]] == [3, 4, 5, 2]                           # the hands past the score vector count as 1.0
    dets, _ = c["outside_frame_max2_iou0.2"].expected()
    assert [int(i) for i in dets["index"]] == [0, 2] and [int(v) for v in dets["has_od"]] == [0, 1]
    dets, _ = c["outside_frame_max4_iou0.2"].expected()
    assert [int(i) for i in dets["index"]] == [0, 2, 3]
    dets, _ = c["outside_frame_max4_iou0.9"].expected()
    assert [int(i) for i in dets["index"]] == [0, 1, 2, 3] and [int(v) for v in dets["has_od"]] == [0, 0, 1, 1]
    dets, _ = c["no_frame"].expected()
    assert [int(v) for v in dets["has_od"]] == [1, 1, 1]
    dets, _ = c["nan_settings"].expected()
    assert [int(i) for i in dets["index"]] == [1, 0, 3, 2]                               # +NaN first, -NaN last
    for case, n in H.landmarks_iou_pair():
        assert len(case.expected()[0]) == n, case.name


def test_unclamped_landmark_threshold():
    hands = np.stack([H.hand_box(100 + 150 * k, 50, 200 + 150 * k, 150) for k in range(3)])
    assert len(R.landmarks_decode(hands, None, 0.5, -1.0, 10, (640, 360))[0]) == 1        # iou 0 > -1: the first hand suppresses all
    assert len(R.landmarks_decode(hands, None, 0.5, 0.0, 10, (640, 360))[0]) == 3


def test_survivor_counts_straddle_the_powers_of_two():
    seen = set()
    for c in H.palm_random():
        if "_k" in c.name and not c.name.endswith("kNone"):
            k = int(c.name.rsplit("_k", 1)[1])
            assert len(R.palm_candidates(c.data, c.params[0], c.params[3])[0]) == k, c.name
            seen.add(k)
    assert {31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025} <= seen
    big = [c for c in H.palm_random() if c.name == "random_N4096_kNone"][0]
    n = len(R.palm_candidates(big.data, -1.0, big.params[3])[0])
    assert 0.35 * 4096 < n < 0.5 * 4096                                                  # about 42 % of the synthetic rows are valid


def test_total_key_is_total_cmp():
    u = np.array([0xFFFFFFFF, H.QNAN_NEG, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0, 1, 0x3F800000, 0x7F800000, 0x7F800001, H.QNAN_POS],
                 np.uint32)
    assert (np.diff(R.total_key(u.view(np.float32)).astype(np.int64)) > 0).all()


# ---------------------------------------------------------------- deviation a's guard

def test_near_tie_flags_midpoints_and_nothing_else():
    a, b = np.float64(F32(1.0)), np.float64(np.nextafter(F32(1.0), F32(2.0)))
    mid = (a + b) / 2
    assert R.near_tie(mid)[0] and R.near_tie(mid + 16 * np.spacing(mid))[0] and not R.near_tie(mid + 40 * np.spacing(mid))[0]
    assert not R.near_tie([a, b, 0.0, np.pi / 2, -np.pi, np.inf, np.nan]).any()


def test_near_tie_flags_no_value_of_any_case():
    for c in H.palm_all():
        assert not R.near_tie(R.palm_trig64(c.data, c.params[0])).any(), c.name
    for c in H.landmarks_all():
        assert not R.near_tie(R.landmarks_trig64(c.data, c.scores, c.params[0])).any(), c.name


# ---------------------------------------------------------------- numpy against C++

@pytest.fixture(scope="module")
def cpu_lib(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++: the C++ restatement cannot be built")
    so = str(tmp_path_factory.mktemp("handdec_cpu") / "libhanddec_cpu.so")
    subprocess.check_call([cxx, "-O3", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tools", "handdec_cpu.cpp"), "-o", so])
    L = C.CDLL(so)
    L.handdec_palm_cpu.restype = C.c_int
    L.handdec_palm_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_uint32)]
    L.handdec_landmarks_cpu.restype = C.c_int
    L.handdec_landmarks_cpu.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    return L


def test_cpp_palm_equals_numpy(cpu_lib):
    for case in H.palm_all():
        dets = np.zeros(10, R.DET)
        n = C.c_uint32(0)
        assert cpu_lib.handdec_palm_cpu(case.data.ctypes.data, case.N, *H.flat_params(case.params), dets.ctypes.data, C.byref(n)) == 0
        want = case.expected()
        assert n.value == len(want) and R.same_records(dets[:n.value], want), case.name


def test_cpp_landmarks_equal_numpy(cpu_lib):
    for case in H.landmarks_all():
        dets, kps = np.zeros(10, R.DET), np.zeros(10, R.KP)
        n = C.c_uint32(0)
        sc = case.scores
        rc = cpu_lib.handdec_landmarks_cpu(case.data.ctypes.data, case.H, case.D, None if sc is None else sc.ctypes.data, 0 if sc is None else len(sc),
                                           *H.flat_params(case.params), dets.ctypes.data, kps.ctypes.data, C.byref(n))
        want_d, want_k = case.expected()
        assert rc == 0 and n.value == len(want_d), case.name
        assert R.same_records(dets[:n.value], want_d) and R.same_records(kps[:n.value], want_k), case.name


# ---------------------------------------------------------------- ABI surface and the checks that need no device

NEW_SYMBOLS = ("mi355_handdec_palm_tensor", "mi355_handdec_palm_tensors_device", "mi355_handdec_landmarks_tensor", "mi355_handdec_landmarks_tensors_device",
               "mi355_selftest_handdec_check")


def test_library_exports_the_entry_points(mi355lib):
    import mi355fx
    hdr = open(mi355fx.HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr and hasattr(mi355lib, name) and getattr(mi355lib, name).argtypes is not None, name
    assert mi355lib.mi355_abi_version() == 1


def test_records_and_params_match_the_header_layout():
    import mi355fx
    assert mi355fx.HAND_DET.itemsize == 64 and mi355fx.HAND_DET == R.DET
    assert [mi355fx.HAND_DET.fields[n][1] for n in ("xmin", "rotation", "rotation_od", "confidence", "index", "x", "has_od", "reserved")] == [0, 16, 20, 24, 28, 32, 48, 52]
    assert mi355fx.HAND_KP.itemsize == 288 and mi355fx.HAND_KP == R.KP
    assert [mi355fx.HAND_KP.fields[n][1] for n in ("count", "positions", "confidences", "visibilities", "reserved")] == [0, 4, 172, 256, 277]
    assert C.sizeof(mi355fx.HandParams) == 20 and mi355fx.HandParams.max_hands.offset == 8 and mi355fx.HandParams.frame_height.offset == 16
    assert mi355fx.HAND_MAX == 10 and mi355fx.KP_VISIBILITY == {"UNKNOWN": R.KP_UNKNOWN, "VISIBLE": R.KP_VISIBLE, "OCCLUDED": R.KP_OCCLUDED}
    hdr = open(mi355fx.HEADER_PATH).read()
    assert "#define MI355_HAND_MAX 10" in hdr and "MI355_KP_UNKNOWN = 0, MI355_KP_VISIBLE = 1, MI355_KP_OCCLUDED = 2" in hdr


def test_shape_and_params_checks(mi355lib):
    import mi355fx
    chk = mi355lib.mi355_selftest_handdec_check
    INV, UNS = mi355fx.ERR_INVALID_ARG, mi355fx.ERR_UNSUPPORTED

    def palm(N, T=1, pitch=None, max_hands=2, frame=(0, 0)):
        return chk(0, N * 32 if pitch is None else pitch, T, N, 0, 0, 0, max_hands, *frame)

    def lm(Hn, D=3, T=1, pitch=None, spitch=None, ns=0, max_hands=2, frame=(640, 360)):
        return chk(1, Hn * 21 * D * 4 if pitch is None else pitch, T, Hn, D, ns * 4 if spitch is None else spitch, ns, max_hands, *frame)

    assert palm(0) == 0 and palm(1) == 0 and palm(4096, 1024) == 0 and palm(4097) == UNS
    assert palm(10, 1025) == UNS and palm(10, 0) == INV and palm(10, -1) == INV
    assert palm(10, 2, 316) == INV and palm(10, 2, 322) == INV and palm(10, 2, 324) == 0       # pitch below the tensor, no multiple of 4, larger
    assert [palm(10, max_hands=m) for m in (0, 1, 8, 9)] == [INV, 0, 0, INV]
    assert [palm(10, frame=f) for f in ((0, 0), (1, 1), (192, 0), (0, 192), (-1, -1), (-1, 5))] == [0, 0, INV, INV, INV, INV]
    assert lm(0) == 0 and lm(1) == 0 and lm(1024, 16, 1024) == 0 and lm(1025) == UNS
    assert [lm(4, D=d) for d in (0, 1, 2, 16, 17)] == [INV, INV, 0, 0, UNS]
    assert lm(4, T=1025) == UNS and lm(4, T=0) == INV
    assert lm(4, 3, 2, 4 * 63 * 4 - 4) == INV and lm(4, 3, 2, 4 * 63 * 4 + 2) == INV and lm(4, 3, 2, 4 * 63 * 4 + 4) == 0
    assert [lm(4, max_hands=m) for m in (0, 1, 10, 11)] == [INV, 0, 0, INV]
    assert lm(4, ns=2) == 0 and lm(4, ns=1024) == 0 and lm(4, ns=1025) == UNS
    assert lm(4, ns=4, spitch=12) == INV and lm(4, ns=4, spitch=18) == INV and lm(4, ns=4, spitch=20) == 0
    assert lm(4, frame=(0, 0)) == 0 and lm(4, frame=(0, 7)) == INV
    assert chk(2, 0, 1, 0, 2, 0, 0, 2, 0, 0) == INV and chk(-1, 0, 1, 0, 2, 0, 0, 2, 0, 0) == INV


def test_null_context_is_refused(mi355lib):
    import mi355fx
    p = mi355fx.HandParams(0.5, 0.2, 2, 0, 0)
    n = C.c_uint32(7)
    assert mi355lib.mi355_handdec_palm_tensor(None, None, 0, C.byref(p), None, C.byref(n)) == mi355fx.ERR_INVALID_ARG
    assert mi355lib.mi355_handdec_palm_tensors_device(None, None, 0, 1, 0, C.byref(p), None, C.byref(n)) == mi355fx.ERR_INVALID_ARG
    assert mi355lib.mi355_handdec_landmarks_tensor(None, None, 0, 3, None, 0, C.byref(p), None, None, C.byref(n)) == mi355fx.ERR_INVALID_ARG
    assert mi355lib.mi355_handdec_landmarks_tensors_device(None, None, 0, 1, 0, 3, None, 0, 0, C.byref(p), None, None, C.byref(n)) == mi355fx.ERR_INVALID_ARG
    assert n.value == 7
