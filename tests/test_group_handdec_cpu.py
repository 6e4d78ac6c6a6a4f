"""CPU companion of tests/test_gpu_group_handdec.py: the surfaces the hand-decoder queue of the video group adds (library exports,
header, bindings, documents) and the layout of one launch set (mi355_selftest_handdec_set_plan: host only, no device), compared with
a restatement in Python."""
import ctypes as C
import os
import re

import pytest

import handdec_group_members as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["mi355_group_set_handdec_rendezvous", "mi355_group_submit_handdec_palm", "mi355_group_submit_handdec_landmarks", "mi355_group_wait_handdec",
             "mi355_group_handdec_stats", "mi355_selftest_handdec_set_plan"]
METHODS = ("set_handdec_rendezvous", "submit_handdec_palm", "submit_handdec_landmarks", "wait_handdec", "handdec_stats")
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED = 0, -1, -6
PALM, LANDMARKS = M.PALM, M.LANDMARKS
NONE = 0xFFFFFFFF                      # UINT32_MAX: no block / no keypoint slot
HAND_MAX, DET_BYTES, KP_BYTES = 10, 64, 288


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
    for name in NEW_NAMES + ["MI355_HANDDEC_SET_MAX"]:
        assert re.search(r"\b%s\b" % name, h), name
    for name in NEW_NAMES:
        assert re.search(r"\b%s\(" % name, h), name
    assert re.search(r"#define MI355_HANDDEC_SET_MAX\s+32\b", h)
    assert re.search(r"#define MI355FX_ABI_VERSION\s+1\b", h)
    assert (ERR_INVALID_ARG, ERR_UNSUPPORTED) == tuple(int(re.search(r"\b%s\s*=\s*(-?\d+)" % n, h).group(1)) for n in ("MI355_ERR_INVALID_ARG", "MI355_ERR_UNSUPPORTED"))


def test_bindings_and_documents_name_every_entry_point():
    py = _read("gst-plugins-rs_amd", "mi355fx", "__init__.py")
    for name in NEW_NAMES:
        assert '"%s"' % name in py, name
        for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
            assert name in _read(doc), (name, doc)
    for method in METHODS:
        assert re.search(r"    def %s\(self" % method, py), method
    assert re.search(r"^def selftest_handdec_set_plan\(", py, flags=re.M)
    assert re.search(r"^HANDDEC_SET_MAX = 32\b", py, flags=re.M)


def test_python_carries_the_methods():
    import mi355fx
    for method in METHODS:
        assert callable(getattr(mi355fx.Group, method))
    assert callable(mi355fx.selftest_handdec_set_plan)
    assert mi355fx.HANDDEC_SET_MAX == 32


def restate(decoder, rows):
    """The plan, restated: jobs in submit order, running counts per decoder."""
    block, kp_slot, with_rows, n_landmarks = [], [], [0, 0], 0
    for d, r in zip(decoder, rows):
        block.append(with_rows[d] if r else NONE)
        with_rows[d] += 1 if r else 0
        kp_slot.append(n_landmarks if d == LANDMARKS else NONE)
        n_landmarks += 1 if d == LANDMARKS else 0
    copied = 128 + len(rows) * HAND_MAX * DET_BYTES + n_landmarks * HAND_MAX * KP_BYTES if sum(with_rows) else 0
    return block, kp_slot, [with_rows[PALM], with_rows[LANDMARKS], n_landmarks, copied]


def _plan(decoder, rows):
    import mi355fx
    return mi355fx.selftest_handdec_set_plan(decoder, rows)


def _mixed():
    spec = M.mixed_spec()
    return [s[0] for s in spec], [s[1] for s in spec]


CASES = {
    "empty": ([], []),
    "mixed": _mixed(),
    "all_empty_tensors": ([PALM, LANDMARKS, PALM, LANDMARKS], [0, 0, 0, 0]),
    "palm32": ([PALM] * 32, [(2016, 1, 0, 4096)[k % 4] for k in range(32)]),
    "landmarks32": ([LANDMARKS] * 32, [(2, 0, 1024, 1)[k % 4] for k in range(32)]),
    "alternating": ([k % 2 for k in range(32)], [(5, 0, 7)[k % 3] for k in range(32)]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_equals_its_restatement(case):
    decoder, rows = CASES[case]
    rc, block, kp_slot, totals = _plan(decoder, rows)
    assert rc == OK
    assert (block, kp_slot, totals) == restate(decoder, rows)


def test_the_cases_are_what_they_are_meant_to_be():
    decoder, rows = _mixed()
    assert 20 <= len(rows) <= 32 and {PALM, LANDMARKS} == set(decoder)
    assert {r for d, r in zip(decoder, rows) if d == PALM} >= {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2016, 4096}
    assert {r for d, r in zip(decoder, rows) if d == LANDMARKS} >= {0, 1, 3, 4, 5, 10, 11, 64}
    for which in (PALM, LANDMARKS):                                           # a job without rows between two with rows, in each decoder
        own = [r for d, r in zip(decoder, rows) if d == which]
        assert any(a and not b and c for a, b, c in zip(own, own[1:], own[2:]))
    assert any(a != b for a, b in zip(decoder, decoder[1:]))
    assert _plan(*CASES["all_empty_tensors"])[3] == [0, 0, 2, 0]
    assert _plan(*CASES["palm32"])[3][:3] == [24, 0, 0] and _plan(*CASES["landmarks32"])[3][:3] == [0, 24, 32]


def test_plan_values_by_hand():
    # palm 2016 | landmarks 2 | palm 0 | landmarks 0 | palm 1 | landmarks 5
    rc, block, kp_slot, totals = _plan([PALM, LANDMARKS, PALM, LANDMARKS, PALM, LANDMARKS], [2016, 2, 0, 0, 1, 5])
    assert rc == OK
    assert block == [0, 0, NONE, NONE, 1, 1]
    assert kp_slot == [NONE, 0, NONE, 1, NONE, 2]
    assert totals == [2, 2, 3, 128 + 6 * 640 + 3 * 2880] == [2, 2, 3, 12608]
    # the slab's maximum: 32 landmark jobs
    assert _plan([LANDMARKS] * 32, [1] * 32)[3] == [0, 32, 32, 128 + 32 * 640 + 32 * 2880]


def test_plan_refusals(lib):
    assert _plan([PALM], [10])[0] == OK
    assert _plan([PALM] * 33, [10] * 33)[0] == ERR_INVALID_ARG
    assert _plan([2], [10])[0] == ERR_INVALID_ARG                             # a decoder that is neither
    assert _plan([PALM, -1], [10, 10])[0] == ERR_INVALID_ARG
    assert _plan([PALM], [4096])[0] == OK and _plan([PALM], [4097])[0] == ERR_UNSUPPORTED
    assert _plan([LANDMARKS], [1024])[0] == OK and _plan([LANDMARKS], [1025])[0] == ERR_UNSUPPORTED
    assert _plan([PALM, LANDMARKS], [1025, 1025])[0] == ERR_UNSUPPORTED       # the second job's refusal
    f = lib.mi355_selftest_handdec_set_plan
    f.restype = C.c_int
    p32 = C.POINTER(C.c_uint32)
    f.argtypes = [C.c_int, C.POINTER(C.c_int), p32, p32, p32, C.POINTER(C.c_uint64)]
    u, totals = lambda v=10: (C.c_uint32 * 1)(v), (C.c_uint64 * 4)()
    full = [(C.c_int * 1)(PALM), u(), u(), u()]
    assert f(1, *full, totals) == OK
    for k in range(len(full)):                                                # every array in turn
        args = list(full)
        args[k] = None
        assert f(1, *args, totals) == ERR_INVALID_ARG, k
    assert f(1, *full, None) == ERR_INVALID_ARG
    assert f(-1, *full, totals) == ERR_INVALID_ARG
    assert f(0, *full, None) == ERR_INVALID_ARG
    assert f(0, *([None] * 4), totals) == OK and list(totals) == [0] * 4
