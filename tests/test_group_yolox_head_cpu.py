"""CPU companion of tests/test_gpu_group_yolox_head.py: the surfaces that yoloxinference's head maps add to the decoder queue of the
video group (library exports, header, bindings, documents) and the layout of one launch set that may hold heads
(mi355_selftest_yolox_head_set_plan: host only, no device), compared with a restatement in numpy and with the tensor-only plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yolox_head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_group_submit_yolox_head", "mi355_group_yolox_head_stats", "mi355_selftest_yolox_head_set_plan"]
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED = 0, -1, -6
V8, X, HEAD = 0, 1, 2


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
    assert re.search(r"#define MI355_YOLO_X_HEAD\s+2\b", h)
    assert re.search(r"#define MI355_YOLODEC_SET_MAX\s+32\b", h)
    # the other queues' wait functions list the head ticket among those they refuse
    assert "a tensor's or a head's" in h


def test_bindings_and_documents_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
            assert name in _read(doc), (name, doc)
    for method in ("submit_yolox_head", "yolox_head_stats"):
        assert re.search(r"    def %s\(self" % method, py), method
    assert re.search(r"^def selftest_yolox_head_set_plan\(", py, flags=re.M)
    assert re.search(r"^YOLO_X_HEAD = 2\b", py, flags=re.M)
    for kernel in ("yolox_head_score_jobs_kernel", "yolox_head_nms_jobs_kernel"):
        assert kernel in _read("DESIGN.md"), kernel
    assert "does not take head maps yet" not in _read("DESIGN.md")
    assert "yolox_head_group_bench.txt" in _read("profiles", "README.md")


def test_python_carries_the_methods():
    import mi355fx
    for method in ("submit_yolox_head", "yolox_head_stats"):
        assert callable(getattr(mi355fx.Group, method))
    assert callable(mi355fx.selftest_yolox_head_set_plan)
    assert mi355fx.YOLO_X_HEAD == HEAD


# ---------------------------------------------------------------- the plan

def restate(kinds, N, max_dets, shapes):
    """The plan, restated with numpy: jobs in submit order, running sums. shapes: per job the (h, w) of a head's levels."""
    cand, first, blocks, key, box, det, lfirst = [], [], [], [], [], [], []
    t = [0] * 8
    for k, n, m, lv in zip(kinds, N, max_dets, shapes):
        if k == HEAD:
            hw = np.array([h * w for h, w in lv], np.int64)
            tiles = (hw + 255) // 256
            n = int(hw.sum())
            b = int(tiles.sum())
            lfirst.append([int(v) for v in np.cumsum(tiles) - tiles])
            first.append(t[6])
            t[6] += b
            t[7] += len(lv)
        else:
            b = -(-n // 256)
            lfirst.append([])
            first.append(t[k])
            t[k] += b
        cand.append(n); blocks.append(b); key.append(t[3]); box.append(t[4]); det.append(t[5])
        t[2] += 1 if n else 0
        t[3] += 1 << max(n - 1, 0).bit_length()      # the power of two at or above n (1 for n = 0)
        t[4] += n
        t[5] += min(m, n)
    return cand, first, blocks, key, box, det, lfirst, t


def _plan(kinds, F, N, max_dets, shapes):
    import mi355fx
    return mi355fx.selftest_yolox_head_set_plan(kinds, F, N, max_dets, shapes)


def _random_set(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 33))
    names = list(H.LEVEL_SETS)
    kinds, F, N, cap, shapes = [], [], [], [], []
    for _ in range(n):
        k = int(rng.integers(0, 3))
        kinds.append(k)
        if k == HEAD:
            if rng.integers(0, 2):
                lv = list(H.LEVEL_SETS[names[int(rng.integers(0, len(names)))]])
            else:
                lv = [(int(rng.integers(1, 90)), int(rng.integers(1, 90))) for _ in range(int(rng.integers(1, 9)))]
            a = sum(h * w for h, w in lv)
            shapes.append(lv)
            N.append(int(rng.integers(0, 70000)))       # ignored for a head
        else:
            a = int(rng.choice([0, 1, 255, 256, 257, 512, 4097, 8400, 65536]))
            shapes.append([])
            N.append(a)
        F.append(int(rng.choice([6, 7, 85, 133, 1029])))
        cap.append(int(rng.choice([0, max(a - 1, 0), a, a + 7])))
    return kinds, F, N, cap, shapes


@pytest.mark.parametrize("seed", range(12))
def test_plan_equals_its_restatement_on_random_mixed_sets(seed):
    import mi355fx
    kinds, F, N, cap, shapes = _random_set(seed)
    rc, *got = _plan(kinds, F, N, cap, shapes)
    assert rc == OK
    want = restate(kinds, N, cap, shapes)
    assert tuple(got) == want
    # the tensor jobs: block ranges as the tensor-only plan lays them out for these tensors alone
    tj = [j for j, k in enumerate(kinds) if k != HEAD]
    rc, first, blocks, _, _, _, totals = mi355fx.selftest_yolodec_set_plan([kinds[j] for j in tj], [F[j] for j in tj], [N[j] for j in tj], [cap[j] for j in tj])
    assert rc == OK
    assert [got[1][j] for j in tj] == first and [got[2][j] for j in tj] == blocks and got[7][:2] == totals[:2]
    # ... and every offset of the jobs in front of the first head
    lead = kinds.index(HEAD) if HEAD in kinds else len(kinds)
    rc, first, blocks, key, box, det, _ = mi355fx.selftest_yolodec_set_plan(kinds[:lead], F[:lead], N[:lead], cap[:lead])
    assert rc == OK
    assert (got[0][:lead], got[1][:lead], got[2][:lead], got[3][:lead], got[4][:lead], got[5][:lead]) == (N[:lead], first, blocks, key, box, det)


def test_a_set_without_a_head_is_the_old_plan():
    import mi355fx
    kinds, F, N, cap = [V8, X, X, V8], [84, 85, 6, 6], [8400, 256, 0, 1], [100, 300, 5, 0]
    rc, cand, first, blocks, key, box, det, lfirst, totals = _plan(kinds, F, N, cap, [[]] * 4)
    old = mi355fx.selftest_yolodec_set_plan(kinds, F, N, cap)
    assert rc == OK and (rc, first, blocks, key, box, det, totals[:6]) == old
    assert cand == N and totals[6:] == [0, 0] and lfirst == [[]] * 4
    assert _plan(kinds, F, N, cap, None)[:7] == (rc, cand, first, blocks, key, box, det)      # no head job: the level arrays may be null
    assert _plan([], [], [], [], [])[0] == OK and _plan([], [], [], [], [])[8] == [0] * 8


def test_plan_values_by_hand():
    # boundary255 (255 + 2 candidates: one tile each) | V8 300 | eight (8 levels of 6: a tile each), head num_candidates ignored
    b255, eight = H.LEVEL_SETS["boundary255"], H.LEVEL_SETS["eight"]
    assert b255 == [(15, 17), (1, 2)] and eight == [(2, 3)] * 8
    rc, cand, first, blocks, key, box, det, lfirst, totals = _plan([HEAD, V8, HEAD], [85, 84, 6], [77777, 300, 0], [10, 1000, 7], [b255, [], eight])
    assert rc == OK
    assert cand == [257, 300, 48]
    assert first == [0, 0, 2] and blocks == [2, 2, 8]                       # the second head's tiles start behind the first head's two
    assert lfirst == [[0, 1], [], [0, 1, 2, 3, 4, 5, 6, 7]]
    assert key == [0, 512, 1024] and box == [0, 257, 557] and det == [0, 10, 310]
    assert totals == [2, 0, 3, 1024 + 64, 257 + 300 + 48, 10 + 300 + 7, 10, 10]


def test_plan_refusals(lib):
    one = [(4, 4)]
    assert _plan([HEAD], [85], [0], [10], [one])[0] == OK
    assert _plan([HEAD] * 33, [85] * 33, [0] * 33, [10] * 33, [one] * 33)[0] == ERR_INVALID_ARG
    assert _plan([3], [85], [0], [10], [one])[0] == ERR_INVALID_ARG                            # no kind
    assert _plan([-1], [85], [0], [10], [one])[0] == ERR_INVALID_ARG
    # a tensor job: the tensor checker's status
    assert _plan([HEAD, V8], [85, 5], [0, 10], [10, 10], [one, []])[0] == ERR_INVALID_ARG
    assert _plan([HEAD, X], [85, 1030], [0, 10], [10, 10], [one, []])[0] == ERR_UNSUPPORTED
    assert _plan([X, HEAD], [6, 85], [65537, 0], [10, 10], [[], one])[0] == ERR_UNSUPPORTED
    # a head job: the head checker's status (test_yolox_head_cpu.py pins these for mi355_selftest_yolox_head_check)
    assert _plan([HEAD], [85], [0], [10], [[]])[0] == ERR_INVALID_ARG                          # no level
    assert _plan([HEAD], [5], [0], [10], [one])[0] == ERR_INVALID_ARG                          # no class
    assert _plan([HEAD], [4], [0], [10], [one])[0] == ERR_INVALID_ARG
    assert _plan([HEAD], [85], [0], [10], [[(4, 4)] * 9])[0] == ERR_UNSUPPORTED                # more than 8 levels
    assert _plan([HEAD], [1030], [0], [10], [one])[0] == ERR_UNSUPPORTED                       # more than 1029 fields
    assert _plan([HEAD], [1029], [0], [10], [one])[0] == OK
    assert _plan([HEAD], [85], [0], [10], [[(4, 4), (0, 3)]])[0] == ERR_INVALID_ARG            # h = 0
    assert _plan([HEAD], [85], [0], [10], [[(4, 4), (3, 0)]])[0] == ERR_INVALID_ARG
    assert _plan([HEAD], [85], [0], [10], [[(256, 256)]])[0] == OK                             # 65536 candidates
    assert _plan([HEAD], [85], [0], [10], [[(256, 256), (1, 1)]])[0] == ERR_UNSUPPORTED
    assert _plan([HEAD], [85], [0], [10], [[(65536, 65536)]])[0] == ERR_UNSUPPORTED            # h * w wraps in 32 bits
    assert _plan([HEAD, HEAD], [85, 85], [0, 0], [10, 10], [one, [(4, 4)] * 9])[0] == ERR_UNSUPPORTED   # the second job's refusal
    # agreement with the checker itself, levels with pointers that are never dereferenced
    import mi355fx
    for lv, Cn in ((one, 80), ([(4, 4)] * 9, 80), ([(256, 256), (1, 1)], 3), ([(4, 4), (0, 3)], 3), (one, 0), (one, 1025)):
        levels = [(64, 64, 64, 4 * h * w * 4, h * w * 4, Cn * h * w * 4, h, w, 8) for h, w in lv]
        A = sum(h * w for h, w in lv)
        assert _plan([HEAD], [5 + Cn], [0], [10], [lv])[0] == mi355fx.selftest_yolox_head_check(levels, 1, Cn, A * (5 + Cn) * 4), (lv, Cn)
    # null arrays, through the C entry itself
    f = lib.mi355_selftest_yolox_head_set_plan
    f.restype = C.c_int
    pi, p32, p64 = C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    f.argtypes = [C.c_int, pi, p32, p32, p32, pi, p32, p32, p32, p32, p32, p64, p64, p64, p32, p64]
    u, q, totals = lambda v=4: (C.c_uint32 * 1)(v), lambda: (C.c_uint64 * 1)(), (C.c_uint64 * 8)()
    full = [(C.c_int * 1)(HEAD), u(85), u(), u(), (C.c_int * 1)(1), u(), u(), u(), u(), u(), q(), q(), q(), u()]
    assert f(1, *full, totals) == OK and list(totals) == [0, 0, 1, 16, 16, 4, 1, 1]
    for k in range(len(full)):                                               # every array in turn
        args = list(full)
        args[k] = None
        assert f(1, *args, totals) == ERR_INVALID_ARG, k
    assert f(1, *full, None) == ERR_INVALID_ARG
    assert f(-1, *full, totals) == ERR_INVALID_ARG
    assert f(33, *full, totals) == ERR_INVALID_ARG
    assert f(0, *full, None) == ERR_INVALID_ARG
    assert f(0, *([None] * 14), totals) == OK and list(totals) == [0] * 8
    tensor = list(full)
    tensor[0], tensor[1] = (C.c_int * 1)(V8), u(6)
    for k in (4, 5, 6, 13):                                                  # a tensor job reads no level array
        tensor[k] = None
    assert f(1, *tensor, totals) == OK and list(totals) == [1, 0, 1, 4, 4, 4, 0, 0]
