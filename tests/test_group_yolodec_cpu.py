"""CPU companion of tests/test_gpu_group_yolodec.py: the surfaces the decoder queue of the video group adds (library exports, header,
bindings, documents) and the layout of one launch set (mi355_selftest_yolodec_set_plan: host only, no device), compared with a
restatement in Python."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_group_set_yolodec_rendezvous", "mi355_group_submit_yolodec", "mi355_group_wait_yolodec", "mi355_group_yolodec_stats",
             "mi355_selftest_yolodec_set_plan"]
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED = 0, -1, -6
V8, X = 0, 1


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(os.path.join(ROOT, "gst-plugins-rs_amd", "libmi355fx.so"))


def test_library_exports_the_new_names(lib):
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
    lib.mi355_abi_version.restype = C.c_int
    assert lib.mi355_abi_version() == 1


def test_header_declares_the_new_names():
    h = _read("include", "mi355fx.h")
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, h), name
    assert re.search(r"#define MI355_YOLODEC_SET_MAX\s+32\b", h)
    assert re.search(r"#define MI355FX_ABI_VERSION\s+1\b", h)
    assert (ERR_INVALID_ARG, ERR_UNSUPPORTED) == tuple(int(re.search(r"\b%s\s*=\s*(-?\d+)" % n, h).group(1)) for n in ("MI355_ERR_INVALID_ARG", "MI355_ERR_UNSUPPORTED"))


def test_bindings_and_documents_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
            assert name in _read(doc), (name, doc)
    for method in ("set_yolodec_rendezvous", "submit_yolodec", "wait_yolodec", "yolodec_stats"):
        assert re.search(r"    def %s\(self" % method, py), method
    assert re.search(r"^def selftest_yolodec_set_plan\(", py, flags=re.M)
    assert re.search(r"^YOLODEC_SET_MAX = 32\b", py, flags=re.M)


def test_python_carries_the_methods():
    import mi355fx
    for method in ("set_yolodec_rendezvous", "submit_yolodec", "wait_yolodec", "yolodec_stats"):
        assert callable(getattr(mi355fx.Group, method))
    assert callable(mi355fx.selftest_yolodec_set_plan)
    assert mi355fx.YOLODEC_SET_MAX == 32


def restate(layout, N, max_dets):
    """The plan, restated: jobs in submit order, running sums."""
    first, blocks, key, box, det = [], [], [], [], []
    t = [0] * 6
    for l, n, m in zip(layout, N, max_dets):
        b = -(-n // 256)
        first.append(t[l]); blocks.append(b); key.append(t[3]); box.append(t[4]); det.append(t[5])
        t[l] += b
        t[2] += 1 if n else 0
        t[3] += 1 << max(n - 1, 0).bit_length()      # the power of two at or above n (1 for n = 0)
        t[4] += n
        t[5] += min(m, n)
    return first, blocks, key, box, det, t


def _plan(layout, F, N, max_dets):
    import mi355fx
    return mi355fx.selftest_yolodec_set_plan(layout, F, N, max_dets)


def _mixed32():
    Ns = [0, 1, 255, 256, 257, 512, 4096, 4097, 65536]
    layout, F, N, cap = [], [], [], []
    for k in range(32):
        n = Ns[k % len(Ns)]
        layout.append((V8, X, X, V8, X)[k % 5])
        F.append((6, 7, 84, 85, 133, 1029)[k % 6])
        N.append(n)
        cap.append((max(n - 1, 0), n, n + 7, 0)[k % 4])     # below, at and above N, and none
    return layout, F, N, cap


CASES = ["empty", "one_v8", "one_x", "mixed32", "all_empty_tensors"]


def _case(case):
    return {
        "empty": ([], [], [], []),
        "one_v8": ([V8], [84], [8400], [100]),
        "one_x": ([X], [85], [8400], [9000]),
        "mixed32": _mixed32(),
        "all_empty_tensors": ([V8, X, V8], [6, 6, 6], [0, 0, 0], [0, 5, 0]),
    }[case]


@pytest.mark.parametrize("case", CASES)
def test_plan_equals_its_restatement(case):
    layout, F, N, cap = _case(case)
    rc, first, blocks, key, box, det, totals = _plan(layout, F, N, cap)
    assert rc == OK
    assert (first, blocks, key, box, det, totals) == restate(layout, N, cap)


@pytest.mark.parametrize("case", CASES)
def test_plan_is_the_mixed_plan_without_heads(case):
    """mi355_selftest_yolodec_set_plan is a thin front of the plan the queue's launch uses (mi355_selftest_yolox_head_set_plan): on
    jobs without a head both give the same five per-job arrays and the same first six totals, and the mixed plan's two head totals
    are zero."""
    import mi355fx
    layout, F, N, cap = _case(case)
    rc, first, blocks, key, box, det, totals = _plan(layout, F, N, cap)
    assert rc == OK
    for levels in ([[] for _ in layout], None):                               # empty level arrays, null level arrays
        mrc, cand, mfirst, mblocks, mkey, mbox, mdet, _, mtotals = mi355fx.selftest_yolox_head_set_plan(layout, F, N, cap, levels)
        assert mrc == OK
        assert cand == N
        assert (first, blocks, key, box, det) == (mfirst, mblocks, mkey, mbox, mdet)
        assert totals == mtotals[:6] and mtotals[6:] == [0, 0]


def test_plan_values_by_hand():
    # V8 8400 | X 256 | V8 0 | X 1: the X job behind a full tile starts at block 1 of its own launch
    rc, first, blocks, key, box, det, totals = _plan([V8, X, V8, X], [84, 85, 6, 6], [8400, 256, 0, 1], [100, 300, 5, 0])
    assert rc == OK
    assert first == [0, 0, 33, 1] and blocks == [33, 1, 0, 1]
    assert key == [0, 16384, 16640, 16641] and box == [0, 8400, 8656, 8656] and det == [0, 100, 356, 356]
    assert totals == [33, 2, 3, 16642, 8657, 356]
    layout, F, N, cap = _mixed32()
    assert {0, 1, 255, 256, 257, 512, 4096, 4097, 65536} == set(N) and set(layout) == {V8, X}
    assert any(c < n for c, n in zip(cap, N)) and any(c == n for c, n in zip(cap, N) if n) and any(c > n for c, n in zip(cap, N))


def test_plan_refusals(lib):
    ok = ([V8], [6], [10], [10])
    assert _plan(*ok)[0] == OK
    assert _plan([V8] * 33, [6] * 33, [10] * 33, [10] * 33)[0] == ERR_INVALID_ARG
    assert _plan([V8], [5], [10], [10])[0] == ERR_INVALID_ARG                 # fewer than 6 fields
    assert _plan([X], [1030], [10], [10])[0] == ERR_UNSUPPORTED               # the checker's own status
    assert _plan([X], [6], [65537], [10])[0] == ERR_UNSUPPORTED
    assert _plan([2], [6], [10], [10])[0] == ERR_INVALID_ARG                  # a bad layout
    assert _plan([V8, -1], [6, 6], [10, 10], [10, 10])[0] == ERR_INVALID_ARG
    assert _plan([V8, X], [6, 1030], [10, 10], [10, 10])[0] == ERR_UNSUPPORTED  # the second job's refusal
    f = lib.mi355_selftest_yolodec_set_plan
    f.restype = C.c_int
    p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    f.argtypes = [C.c_int, C.POINTER(C.c_int), p32, p32, p32, p32, p32, p64, p64, p64, p64]
    lay, u, q, totals = (C.c_int * 1)(V8), lambda v=10: (C.c_uint32 * 1)(v), lambda: (C.c_uint64 * 1)(), (C.c_uint64 * 6)()
    full = [lay, u(6), u(), u(), u(), u(), q(), q(), q()]
    assert f(1, *full, totals) == OK
    for k in range(len(full)):                                               # every array in turn
        args = list(full)
        args[k] = None
        assert f(1, *args, totals) == ERR_INVALID_ARG, k
    assert f(1, *full, None) == ERR_INVALID_ARG
    assert f(-1, *full, totals) == ERR_INVALID_ARG
    assert f(0, *full, None) == ERR_INVALID_ARG
    assert f(0, *([None] * 9), totals) == OK and list(totals) == [0] * 6


def test_plan_refuses_a_head_job_and_writes_nothing(lib):
    """A job of kind MI355_YOLO_X_HEAD is no layout of this plan: MI355_ERR_INVALID_ARG, wherever it stands, and no output is touched."""
    import mi355fx
    assert mi355fx.YOLO_X_HEAD == 2
    f = lib.mi355_selftest_yolodec_set_plan
    f.restype = C.c_int
    p32, p64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    f.argtypes = [C.c_int, C.POINTER(C.c_int), p32, p32, p32, p32, p32, p64, p64, p64, p64]
    mark32, mark64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
    for kinds in ([mi355fx.YOLO_X_HEAD], [V8, mi355fx.YOLO_X_HEAD, X]):
        n = len(kinds)
        lay, F, N, cap = (C.c_int * n)(*kinds), (C.c_uint32 * n)(*[85] * n), (C.c_uint32 * n)(*[8400] * n), (C.c_uint32 * n)(*[100] * n)
        out32 = [(C.c_uint32 * n)(*[mark32] * n) for _ in range(2)]
        out64 = [(C.c_uint64 * n)(*[mark64] * n) for _ in range(3)]
        totals = (C.c_uint64 * 6)(*[mark64] * 6)
        assert f(n, lay, F, N, cap, *out32, *out64, totals) == ERR_INVALID_ARG
        assert all(list(a) == [mark32] * n for a in out32) and all(list(a) == [mark64] * n for a in out64)
        assert list(totals) == [mark64] * 6
        assert _plan(kinds, [85] * n, [8400] * n, [100] * n)[0] == ERR_INVALID_ARG
